// Stream placement (streams.h): the reservation pattern and the per-role rule first -- host
// arithmetic only -- then the HIP side that opens and closes what a plan says.
#include "streams.h"

#include <algorithm>

#include "env.h"

namespace wdr {

std::vector<uint32_t> cu_mask(int ncu, int n_res, int pat, bool only_reserved, std::string* err) {
  auto fail = [&](const char* msg) {
    if (err) *err = msg;
    return std::vector<uint32_t>();
  };
  std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
  if (only_reserved && !(ncu == 256 && n_res > 0 && n_res <= 32 && n_res % 8 == 0)) {
    for (int c = 0; c < ncu; ++c) mask[c / 32] |= 1u << (c % 32);   // no pattern-1 pool to complement
    return mask;
  }
  const bool spread = only_reserved || (pat == 1 && ncu == 256);
  if (!only_reserved) {
    if (n_res >= ncu) return fail("masked stream: must leave at least one CU");
    if (spread && !(n_res % 8 == 0 && n_res <= 32)) return fail("WDR_ENC_MASK_PAT=1: 0, 8, 16, 24 or 32 CUs");
  }
  std::vector<char> res(ncu, 0);
  if (spread) {
    for (int x = 0; x < 8; ++x)
      for (int j = 0; j < std::max(0, n_res) / 8; ++j) res[32 * x + 8 * j + x] = 1;
  } else {
    for (int c = ncu - std::max(0, n_res); c < ncu; ++c) res[c] = 1;
  }
  for (int c = 0; c < ncu; ++c)
    if ((res[c] != 0) == only_reserved) mask[c / 32] |= 1u << (c % 32);
  return mask;
}

StreamKnobs stream_knobs_env() {
  const StreamKnobs def;
  StreamKnobs k;
  k.enc_pool = env_int("WDR_ENC_POOL", def.enc_pool);
  k.enc_mask = env_int("WDR_ENC_MASK", def.enc_mask);
  k.enc_mask_pat = env_int("WDR_ENC_MASK_PAT", def.enc_mask_pat);
  k.enc_prio = env_int("WDR_ENC_PRIO", def.enc_prio);
  k.own_pool = env_int("WDR_OWN_POOL", def.own_pool);
  k.own_mask = env_int("WDR_OWN_MASK", def.own_mask);
  k.own_prio = env_int("WDR_OWN_PRIO", def.own_prio);
  k.odm_pool = env_int("WDR_ODM_POOL", def.odm_pool);
  k.odm_mask = env_int("WDR_ODM_MASK", def.odm_mask);
  k.batch_hwq = env_int("WDR_BATCH_HWQ", def.batch_hwq);
  k.dtwq_hwq = env_int("WDR_DTWQ_HWQ", def.dtwq_hwq);
  k.enc_pool_set = env_set("WDR_ENC_POOL");
  k.enc_mask_set = env_set("WDR_ENC_MASK");
  k.odm_pool_set = env_set("WDR_ODM_POOL");
  return k;
}

StreamPlan stream_plan(StreamRole role, int ncu, const StreamKnobs& k) {
  StreamPlan p;
  auto priority = [&](StreamPrio prio, const char* tag) {
    p.kind = StreamKind::Priority;
    p.prio = prio;
    p.tag = tag;
  };
  // A stream of a pool of `pool` CU-masked streams (dedicated hardware queues) per (tag, device),
  // handed out round-robin, that leave n_res CUs free.  pool <= 0: a stream of its own.
  auto masked = [&](const char* tag, int n_res, int pool) {
    p.kind = StreamKind::Masked;
    p.tag = tag;
    p.pool = std::max(0, pool);
    p.mask = cu_mask(ncu, n_res, k.enc_mask_pat, false, &p.error);
  };
  // A stream on a hardware queue of its own.  HIP multiplexes the process's streams onto at most
  // GPU_MAX_HW_QUEUES (4) hardware queues per priority level, in order: a kernel of the step
  // batcher then waits behind whatever another stream sharing its queue has in front of it (an
  // encoder GEMM launch, a barrier packet waiting on a slot event).  A stream created with a CU
  // mask gets a dedicated queue; the mask here is every CU of the device.  knob 0 (the default
  // of both callers): the shared priority pool.  knob 2 (A/B, MI355X): only the CUs the
  // encode-ahead pool leaves free (WDR_ENC_MASK under WDR_ENC_MASK_PAT=1: 4 per XCD), so this
  // stream's workgroups never wait behind encoder tiles.
  auto dedicated = [&](int knob, StreamPrio prio, const char* tag) {
    if (knob == 0) return priority(prio, tag);
    p.tag = tag;
    p.mask = cu_mask(ncu, knob == 2 ? k.enc_mask : 0, 1, true);
    int n = 0;
    for (uint32_t w : p.mask) n += __builtin_popcount(w);
    p.kind = n == ncu ? StreamKind::MaskedAll : StreamKind::Masked;
  };
  switch (role) {
    case StreamRole::Context:
      // the latency-bound decode chain runs at the highest priority; the encode-ahead stream
      // (State) fills the CUs it leaves idle
      priority(StreamPrio::Highest, "context");
      break;
    case StreamRole::StepBatcher: dedicated(k.batch_hwq, StreamPrio::Highest, "WDR_BATCH_HWQ"); break;
    case StreamRole::DtwQueue: dedicated(k.dtwq_hwq, StreamPrio::Lowest, "WDR_DTWQ_HWQ"); break;
    case StreamRole::StateOwn:
      // Every state has its own highest-priority decode stream (chains run concurrently);
      // WDR_OWN_PRIO=1|2 (A/B): at no / the lowest priority.  WDR_OWN_POOL=P (A/B): the states'
      // own streams from P masked streams (WDR_OWN_MASK CUs left free, default 0) instead, so no
      // chain's own work (on-demand encodes, fix-up passes) shares the step batcher's hardware
      // queue.
      if (k.own_pool >= 0) masked("own", k.own_mask, k.own_pool);
      else priority(k.own_prio == 1 ? StreamPrio::None : k.own_prio == 2 ? StreamPrio::Lowest : StreamPrio::Highest, "");
      break;
    case StreamRole::StateEncAhead: {
      // The encode-ahead streams of all states: WDR_ENC_POOL (default 2) CU-masked streams per
      // device, a dedicated hardware queue each, shared round-robin by the states, which leave
      // WDR_ENC_MASK (default 32) CUs -- 4 per XCD -- to the decode chain.  1-h bench, A/B on one
      // box (profiles/r03/ab_enc_queues.txt): 608-619 xRT with one low-priority stream per state
      // (24 streams on HIP's 4 shared low-priority queues) against 642-646 with 2 or 3 masked
      // queues; 4 or 8 masked queues 576, one 547 (the encoder starves), 24 (one per state) 398.
      // Both knobs -1, or a device other than the 256-CU one this was tuned on with neither knob
      // set: one stream per state at the lowest priority (WDR_ENC_PRIO=1: the middle of the
      // range, 2: the highest; A/B runs).
      const bool plain = (k.enc_mask < 0 && k.enc_pool < 0) || (ncu != 256 && !k.enc_mask_set && !k.enc_pool_set);
      if (!plain) masked("enc", k.enc_mask, k.enc_pool);
      else priority(k.enc_prio == 2 ? StreamPrio::Highest : k.enc_prio == 1 ? StreamPrio::Middle : StreamPrio::Lowest, "");
      break;
    }
    case StreamRole::StateOnDemand:
      // WDR_ODM_POOL (default 4): a long segment's later windows (encoded on demand: they depend
      // on the decoded seek) run on P CU-masked streams (dedicated hardware queues, WDR_ODM_MASK
      // CUs left free, default 32 as the encode-ahead pool), not on the state's own
      // highest-priority stream.  A window's encoder (~70 launches, several ms) on the state
      // stream shared a hardware queue with the step batcher, which runs its packets in order, so
      // every batched step queued behind it waited (configs[2]'s VAD line: long merged segments;
      // profiles/r05/vad_line_queues.txt, profiles/r06/ab_lines_hwq.txt).  -1, or another device
      // than the 256-CU one with the knob unset: the state stream (as before).
      if (k.odm_pool >= 0 && (ncu == 256 || k.odm_pool_set)) masked("odm", k.odm_mask, k.odm_pool);
      break;
    case StreamRole::StateDtw: priority(StreamPrio::Lowest, "state-sd"); break;
  }
  return p;
}

}  // namespace wdr

#ifndef WDR_HOST_ONLY
#include <chrono>
#include <map>
#include <memory>
#include <thread>

#include "prof.h"
#include "whisper.h"

namespace wdr {

using StreamPools = std::map<std::pair<std::string, int>, std::pair<std::vector<hipStream_t>, int>>;
static std::mutex& stream_pools_mu() {
  static std::mutex mu;
  return mu;
}
static StreamPools& stream_pools() {
  static StreamPools* p = new StreamPools();   // outlives static destruction (exit hook)
  return *p;
}

void destroy_stream_pools() {
  std::lock_guard<std::mutex> g(stream_pools_mu());
  for (auto& kv : stream_pools()) {
    (void)hipSetDevice(kv.first.second);
    for (hipStream_t st : kv.second.first) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  }
  stream_pools().clear();
  (void)hipGetLastError();
}

static hipStream_t create_stream(const StreamPlan& p) {
  hipStream_t s = nullptr;
  if (p.kind == StreamKind::Priority && p.prio == StreamPrio::None) {
    WDR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  } else if (p.kind == StreamKind::Priority) {
    int lo = 0, hi = 0;
    WDR_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const int prio = p.prio == StreamPrio::Lowest ? lo : p.prio == StreamPrio::Middle ? (lo + hi) / 2 : hi;
    WDR_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio));
  } else {
    WDR_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)p.mask.size(), p.mask.data()));
  }
  if (!p.tag.empty()) stream_note(p.tag.c_str(), s);
  return s;
}

StreamRef open_stream(const StreamPlan& p) {
  WDR_CHECK(p.error.empty(), p.error);
  StreamRef r;
  if (p.kind == StreamKind::None) return r;
  if (p.kind != StreamKind::Masked || p.pool <= 0) {
    r.s = create_stream(p);
    return r;
  }
  int dev = 0;
  WDR_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(stream_pools_mu());
  auto& P = stream_pools()[{p.tag, dev}];
  if (P.first.empty())
    for (int i = 0; i < p.pool; ++i) P.first.push_back(create_stream(p));
  r.shared = true;
  r.s = P.first[P.second++ % p.pool];
  return r;
}

StreamRef open_stream(StreamRole role, const StreamKnobs& k) {
  int dev = 0, ncu = 0;
  WDR_HIP(hipGetDevice(&dev));
  WDR_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  return open_stream(stream_plan(role, ncu, k));
}

void close_stream(StreamRef& r) {
  if (!r.s) return;
  (void)hipStreamSynchronize(r.s);
  if (!r.shared) (void)hipStreamDestroy(r.s);
  r = StreamRef();
}

// One mutex per pooled stream: a state's encode batch is issued onto a shared stream as one
// unit, so batches run one after another instead of interleaving kernel by kernel (at the start
// of a run every state issues its first batch at once: interleaved, all 12 batches of a stream
// finished together, ~0.6 s in; one after another, the first chains start decoding ~50 ms in).
std::mutex& stream_issue_mutex(hipStream_t st) {
  static std::mutex mu;
  static std::map<hipStream_t, std::unique_ptr<std::mutex>> m;
  std::lock_guard<std::mutex> g(mu);
  auto& p = m[st];
  if (!p) p = std::make_unique<std::mutex>();
  return *p;
}

hipStream_t prime_queue(StreamPrio prio, const char* tag, float* sink) {
  StreamPlan p;
  p.kind = StreamKind::Priority;
  p.prio = prio;
  p.tag = tag ? tag : "";
  const hipStream_t s = create_stream(p);
  if (sink) {
    launch_busy(1, 1000, sink, s);
  } else {
    DevMem one(16);
    WDR_HIP(hipMemsetAsync(one.p, 0, 16, s));
    WDR_HIP(hipStreamSynchronize(s));
  }
  return s;
}

// A chain's wait for its encoded window: hipEventQuery every WDR_READY_POLL_US (default 50 us)
// with the thread asleep in between, instead of hipEventSynchronize, which spins.  At a run's
// start all 40 chains wait for their first encode batches together (0.1-0.6 s in); spinning, they
// spent the process's CPU quota (16 CPUs a 100-ms period on the box) in each of those periods and
// the kernel froze every thread of the process for the rest of it -- 5 throttled periods in a row
// (bench.py host_cpu.throttle_at_s).  0: hipEventSynchronize.
void wait_event_polled(hipEvent_t ev) {
  static const int us = env_int("WDR_READY_POLL_US", 50);
  if (us <= 0) {
    WDR_HIP(hipEventSynchronize(ev));
    return;
  }
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return;
    if (q != hipErrorNotReady) WDR_HIP(q);
    std::this_thread::sleep_for(std::chrono::microseconds(us));
  }
}

// WDR_HOST_FENCE (default 1): a state's own (decode) stream does not carry barrier packets.  HIP
// maps the 40 states' highest-priority streams and the step batcher's onto GPU_MAX_HW_QUEUES
// shared hardware queues, and a queue runs its packets in order: a hipStreamWaitEvent on a state
// stream waiting for a low-priority DTW pass held back every batched step queued behind it on
// that queue (configs[2]'s VAD line: long segments, windows encoded on demand on the state
// stream after such a wait; profiles/r05/vad_line_queues.txt).  The chain's host thread waits
// for the event instead -- it synchronises on that stream right after anyway.
bool host_fence() {
  static const bool v = env_on("WDR_HOST_FENCE", true);
  return v;
}

void stream_fence(hipStream_t s, hipEvent_t ev, bool host) {
  if (host)
    WDR_HIP(hipEventSynchronize(ev));
  else
    WDR_HIP(hipStreamWaitEvent(s, ev, 0));
}

hipGraphExec_t capture_exec(hipStream_t stream, const std::function<void()>& body) {
  std::lock_guard<std::recursive_mutex> cap_lock(hip_alloc_mutex());   // no allocation meanwhile
  hipGraph_t graph;
  prof_capture(true);
  WDR_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
  try {
    body();
  } catch (...) {
    hipGraph_t dead = nullptr;
    (void)hipStreamEndCapture(stream, &dead);
    if (dead) (void)hipGraphDestroy(dead);
    prof_capture(false);
    throw;
  }
  prof_capture(false);
  WDR_HIP(hipStreamEndCapture(stream, &graph));
  hipGraphExec_t exec = nullptr;
  WDR_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  WDR_HIP(hipGraphDestroy(graph));
  return exec;
}

void replay(hipGraphExec_t exec, hipStream_t stream) {
  std::mutex* mu = launch_lock();   // WDR_LAUNCH_LOCK (prof.h)
  if (mu) mu->lock();
  const hipError_t ge = hipGraphLaunch(exec, stream);
  if (mu) mu->unlock();
  WDR_HIP(ge);
}

}  // namespace wdr
#endif
