// Stream placement: which kind of stream each piece of the pipeline runs on (priority, CU mask,
// dedicated hardware queue) as a pure function of the role, the device's CU count and the
// placement knobs, and one way to open and close what the plan says.  The pure part makes no HIP
// call and builds with the host compiler alone (WDR_HOST_ONLY; `make stream-plan-check`,
// tests/test_stream_plan.py through wdr_dbg_cu_mask / wdr_dbg_stream_plan).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace wdr {

// ------------------------------------------------------------------ pure part
// The CU mask of a stream that leaves n_res (< 0: none) of the device's ncu CUs free: one bit per
// CU, (ncu + 31) / 32 words.  pat 1 on a 256-CU device spreads the reserved CUs over the 8 XCDs
// whether mask bit c is CU c % 32 of XCD c / 32 or CU c / 8 of XCD c % 8 -- bits 32x + 8j + x,
// j < n_res / 8 -- since a decode launch's workgroups go round-robin over the XCDs, every XCD
// needs free CUs; otherwise the top n_res bits are reserved.  only_reserved: the complement, the
// CUs such a pool leaves free -- always pattern 1, and every CU unless ncu == 256 and n_res is 8,
// 16, 24 or 32.  On error the result is empty and *err says why.
std::vector<uint32_t> cu_mask(int ncu, int n_res, int pat, bool only_reserved, std::string* err = nullptr);

// Every placement knob as the environment sets it.  The *_set flags carry
// "unset" for the gates that open on a knob being set at all, whatever its value.
struct StreamKnobs {
  int enc_pool = 2, enc_mask = 32, enc_mask_pat = 1, enc_prio = 0;
  int own_pool = -1, own_mask = 0, own_prio = 0;
  int odm_pool = 4, odm_mask = 32;
  int batch_hwq = 0, dtwq_hwq = 0;
  bool enc_pool_set = false, enc_mask_set = false, odm_pool_set = false;
};
StreamKnobs stream_knobs_env();

enum class StreamRole { Context, StepBatcher, DtwQueue, StateOwn, StateEncAhead, StateOnDemand, StateDtw };
enum class StreamKind {
  None,       // no stream: the on-demand role then runs on the state's own stream
  Priority,   // hipStreamCreateWithPriority, or hipStreamCreateWithFlags at StreamPrio::None
  Masked,     // hipExtStreamCreateWithCUMask over `mask`: a dedicated hardware queue
  MaskedAll,  // the same over every CU
};
// None is a stream created without a priority; HIP pools hardware queues per priority, so it is
// not the same as Middle
enum class StreamPrio { Lowest, Middle, Highest, None };

struct StreamPlan {
  StreamKind kind = StreamKind::None;
  StreamPrio prio = StreamPrio::None;
  std::vector<uint32_t> mask;   // Masked / MaskedAll
  std::string tag;              // WDR_STREAM_LOG name at creation ("": not logged) and the pool's key
  int pool = 0;                 // Masked: P > 0 streams per (tag, device) handed out round-robin; 0: its own
  std::string error;            // not empty: the knobs ask for something impossible (open_stream throws it)
};
StreamPlan stream_plan(StreamRole role, int ncu, const StreamKnobs& k);

}  // namespace wdr

#ifndef WDR_HOST_ONLY
// ------------------------------------------------------------------ HIP part
#include <functional>
#include <mutex>

#include "common.h"

namespace wdr {

struct StreamRef {
  hipStream_t s = nullptr;
  bool shared = false;   // from a pool: closed by destroy_stream_pools, not by its user
  operator hipStream_t() const { return s; }
};
// The plan of `role` on the current device from `k`, opened.
StreamRef open_stream(StreamRole role, const StreamKnobs& k);
StreamRef open_stream(const StreamPlan& plan);
// synchronise, then destroy unless shared; the reference is null afterwards
void close_stream(StreamRef& r);
// destroys the process-wide pools of CU-masked streams (wdr_shutdown; no context may be alive)
void destroy_stream_pools();
std::mutex& stream_issue_mutex(hipStream_t st);

// A stream at `prio` whose hardware queue exists from here on: created and given its first work.
// sink null: a 16-byte memset, waited for.  Else one 1-block launch_busy into sink, not waited for
// (WDR_PRIME_POOLS primes 12 queues, then waits for all of them).
hipStream_t prime_queue(StreamPrio prio, const char* tag = nullptr, float* sink = nullptr);

void wait_event_polled(hipEvent_t ev);
bool host_fence();
void stream_fence(hipStream_t s, hipEvent_t ev, bool host);

// `body`'s launches on `stream` as an instantiated graph.  Capture is serialised with allocation
// (hip_alloc_mutex, whisper.h), relaxed, and hidden from the live profiler; if body throws, the
// capture is ended and its graph dropped before the exception goes on.
hipGraphExec_t capture_exec(hipStream_t stream, const std::function<void()>& body);
// one replay, through WDR_LAUNCH_LOCK (prof.h)
void replay(hipGraphExec_t exec, hipStream_t stream);

}  // namespace wdr
#endif
