// Environment knobs: the only place in csrc that reads the environment.  Each
// helper reads at the moment it is called; a site that reads once per process keeps its value
// in a function-local static, a constructor reads per object.  tests/test_cpu_host.py checks
// that the names passed to these helpers and the table in INTEGRATION.md agree.
#pragma once

#include <cstdlib>

namespace wdr {

// the variable as set, or null
inline const char* env_str(const char* name) { return getenv(name); }
// present at all, whatever its value
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline int env_int(const char* name, int def) {
  const char* e = getenv(name);
  return e ? atoi(e) : def;
}
inline double env_double(const char* name, double def) {
  const char* e = getenv(name);
  return e ? atof(e) : def;
}
// def = true: on unless set to 0; def = false: on iff set and not 0
inline bool env_on(const char* name, bool def) {
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : def;
}

}  // namespace wdr
