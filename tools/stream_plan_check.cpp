// Stand-alone check of the pure part of stream placement (csrc/streams.cpp built with
// WDR_HOST_ONLY, csrc/env.h), meant to be built with -fsanitize=address,undefined
// (make -C whisper-diarize-rs_amd stream-plan-check).  Host code only: no HIP, no GPU.
//
// cu_mask and stream_plan over the grid of tests/test_stream_plan.py (and a margin around it):
// every mask has ncu - max(0, n_res) bits and none past ncu, the only_reserved mask is the
// complement of the pool's, an impossible request comes back empty with a message, and every
// role has a plan under every knob setting, from explicit knobs and from the environment.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../whisper-diarize-rs_amd/csrc/streams.h"

using namespace wdr;

static long g_cases = 0;

static void require(bool ok, const char* what, int ncu, int n_res, int pat) {
  ++g_cases;
  if (ok) return;
  fprintf(stderr, "stream_plan_check: %s (ncu %d, n_res %d, pat %d)\n", what, ncu, n_res, pat);
  exit(1);
}

static int bits(const std::vector<uint32_t>& m) {
  int n = 0;
  for (uint32_t w : m) n += __builtin_popcount(w);
  return n;
}

int main() {
  for (int ncu : {256, 304, 64, 40, 1, 33}) {
    for (int pat : {0, 1}) {
      for (int n_res = -9; n_res <= ncu + 1; ++n_res) {
        std::string err;
        const std::vector<uint32_t> m = cu_mask(ncu, n_res, pat, false, &err);
        const bool bad = n_res >= ncu || (pat == 1 && ncu == 256 && (n_res % 8 != 0 || n_res > 32));
        require(m.empty() == bad && err.empty() == !bad, "error cases", ncu, n_res, pat);
        if (bad) continue;
        require((int)m.size() == (ncu + 31) / 32, "mask words", ncu, n_res, pat);
        require(bits(m) == ncu - (n_res > 0 ? n_res : 0), "popcount", ncu, n_res, pat);
        require(ncu % 32 == 0 || (m.back() >> (ncu % 32)) == 0, "bits past ncu", ncu, n_res, pat);
        const std::vector<uint32_t> r = cu_mask(ncu, n_res, 1, true);
        const bool pool = ncu == 256 && n_res > 0 && n_res <= 32 && n_res % 8 == 0;
        require(bits(r) == (pool ? n_res : ncu), "only_reserved popcount", ncu, n_res, pat);
        if (pool && pat == 1)
          for (size_t w = 0; w < m.size(); ++w) require((m[w] ^ r[w]) == 0xffffffffu, "complement", ncu, n_res, pat);
      }
    }
  }
  const int vals[] = {-1, 0, 1, 2, 3, 8, 12, 32, 400};
  for (int ncu : {256, 304, 40})
    for (int role = 0; role <= (int)StreamRole::StateDtw; ++role)
      for (int a : vals)
        for (int b : vals)
          for (int set = 0; set < 2; ++set) {
            StreamKnobs k;
            k.enc_pool = k.own_pool = k.odm_pool = a;
            k.enc_mask = k.own_mask = k.odm_mask = b;
            k.enc_prio = k.own_prio = k.batch_hwq = k.dtwq_hwq = a;
            k.enc_mask_pat = b & 1;
            k.enc_pool_set = k.enc_mask_set = k.odm_pool_set = set != 0;
            const StreamPlan p = stream_plan((StreamRole)role, ncu, k);
            const bool masked = p.kind == StreamKind::Masked || p.kind == StreamKind::MaskedAll;
            require(!p.error.empty() || p.mask.size() == (masked ? (size_t)(ncu + 31) / 32 : 0), "plan mask", ncu, a, b);
            require(p.kind != StreamKind::MaskedAll || bits(p.mask) == ncu, "all CUs", ncu, a, b);
          }
  setenv("WDR_ENC_POOL", "3", 1);
  setenv("WDR_ODM_POOL", "-1", 1);
  const StreamKnobs e = stream_knobs_env();
  require(e.enc_pool == 3 && e.enc_pool_set && !e.enc_mask_set && e.odm_pool == -1 && e.odm_pool_set, "knobs from env", 0, 0, 0);
  require(stream_plan(StreamRole::StateEncAhead, 304, e).pool == 3, "gate opens on a set knob", 304, 0, 0);
  require(stream_plan(StreamRole::StateOnDemand, 256, e).kind == StreamKind::None, "on-demand off", 256, 0, 0);
  printf("stream_plan_check: %ld checks passed\n", g_cases);
  return 0;
}
