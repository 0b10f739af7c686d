// nmpc_probe.h -- the probes of the instrumented builds, and the only file that tests their switches.  The kernels call the hooks below
// unconditionally; in the product they are empty.  The hooks are macros: a call of an inline function alone moves registers (the callee is
// optimised on its own before it is inlined), and a probe must leave the code it measures as it is.
//   -DNMPC_TL         scripts/timeline.py: s_memtime of fifteen events of a helped iteration -- owner 0..10, the helper of its first task
//                     11..14 -- for 64 consecutive iterations of the instance that runs them (one instance solved alone)
//   -DNMPC_PROF2      scripts/sections.py: cycles of each instance by section of the hybrid kernel's loop (=2: of the evaluation), in place
//                     of its status fields.  Every reading drains the LDS queue, so the sum is a little above the plain build's time
//   -DNMPC_MARKS      scripts/isa_stats.py: the sections (with -DNMPC_TL: the timeline events) as markers in the ISA dump
//   -DNMPC_WIN_STATS  scripts/win_stats.py: how often the cross-track window and the obstacle certificate were tried and failed
//   -DNMPC_BBCOUNT    scripts/bbcount.py: one counter per basic block of one solve kernel.  The increments are not in this source:
//                     bbcount.py rewrites the compiler's assembly (four instructions at the head of every block, registers the kernel does
//                     not use) and links the result against nmpc_bbcnt.
#pragma once

namespace nmpc {

// one marker spelling for the ISA dump: fenced by scheduling barriers, or (LOOSE) where the scheduler puts it
#ifdef NMPC_MARKS
#define NMPC_MARK_LOOSE(name) asm volatile("; MARK " #name)
#define NMPC_MARK(name) do { __builtin_amdgcn_sched_barrier(0); NMPC_MARK_LOOSE(name); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define NMPC_MARK_LOOSE(name) do { } while (0)
#define NMPC_MARK(name) do { } while (0)
#endif
// keep-alive: x is computed, in a register, before the probe that follows
#define NMPC_KEEP_ALIVE(x) do { double keep_ = (x); asm volatile("" : "+v"(keep_)); } while (0)

// the per-instance probe state: locals of the hybrid kernel's instance loop, which the hooks below name
#define NMPC_PROBE_STATE NMPC_TL_STATE NMPC_SEC_STATE

// timeline: NMPC_TL_EV(it, ev) = event ev of the owner's PANOC step it (or of its helper), NMPC_TL_KEEP(x) = keep-alive for the next event.
// The owner counts its steps in tl_it and hands the count to the helpers of its request in parameter slot 22 of its slice (NMPC_TL_PUBLISH);
// NMPC_TL_HELPER(Lw, k) declares tl_h, the step of the owner whose slice is Lw as seen by the helper of its task k (-1: task k > 0).
#ifdef NMPC_TL
__device__ long long nmpc_tl[64 * 16];
#ifdef NMPC_MARKS
#define NMPC_TL_EV(it, ev) do { (void)(it); NMPC_MARK(TL_##ev); } while (0)
#else
#define NMPC_TL_EV(it, ev) do { if ((it) >= 200 && (it) < 264 && lane == 0) nmpc_tl[((it) - 200) * 16 + (ev)] = __builtin_amdgcn_s_memtime(); } while (0)
#endif
#define NMPC_TL_STATE int tl_it = 0;
#define NMPC_TL_KEEP(x) NMPC_KEEP_ALIVE(x)
#define NMPC_TL_STEP() tl_it++
#define NMPC_TL_PUBLISH(Lpar) do { if (lane == 0) (Lpar)[22] = (double)tl_it; } while (0)
#define NMPC_TL_HELPER(Lw, k) const int tl_h = (k) == 0 ? (int)(Lw)[mp.par + 22] : -1;
#else
#define NMPC_TL_EV(it, ev) do { } while (0)
#define NMPC_TL_STATE
#define NMPC_TL_KEEP(x) do { } while (0)
#define NMPC_TL_STEP() do { } while (0)
#define NMPC_TL_PUBLISH(Lpar) do { } while (0)
#define NMPC_TL_HELPER(Lw, k)
#endif

// sections: NMPC_SEC(i) ends section i of the loop -- 0 phase handlers in front of the batch, 1 the batch of inner products, 2 exit test / L-BFGS
// update, 3 the recurrences and the direction, 4 envelope, trial points, request, 5 the evaluation, 6 the consumption of the trials -- timed into
// pf<i>; NMPC_SEC_KEEP(x) = keep-alive for it.  NMPC_EVTICK(pe, i) ends section i of an evaluation (NMPC_PROF2 == 2), timed into the caller's
// pe = NMPC_EVAL_PE after NMPC_EVAL_START (or not: nullptr); pe[7] = the last reading.  NMPC_PROBE_STATUS(s): the status of a finished
// instance carries the cycles instead, in the order of the sections (the last / 64).
#ifdef NMPC_PROF2
#define NMPC_STAMP(v) do { __builtin_amdgcn_sched_barrier(0); v = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xc07f); __builtin_amdgcn_sched_barrier(0); } while (0)
#define NMPC_SEC_STATE long long pf0 = 0, pf1 = 0, pf2 = 0, pf3 = 0, pf4 = 0, pf5 = 0, pf6 = 0, pf_last; long long pe[8] = {0, 0, 0, 0, 0, 0, 0, 0}; NMPC_STAMP(pf_last);
#define NMPC_SEC(i) do { long long t_; NMPC_STAMP(t_); pf##i += t_ - pf_last; pf_last = t_; } while (0)
#define NMPC_SEC_KEEP(x) NMPC_KEEP_ALIVE(x)
#define NMPC_PROBE_STATUS_(s, v0, v1, v2, v3, v4, v5, v6) do { (s).last_problem_norm_fpr = (double)(v0); (s).delta_y_norm_over_c = (double)(v1); \
    (s).f2_norm = (double)(v2); (s).penalty = (double)(v3); (s).cost = (double)(v4); (s).solve_time_ms = (double)(v5); (s).num_cost_evals = (uint32_t)((v6) / 64); } while (0)
#else
#define NMPC_SEC_STATE
#define NMPC_SEC(i) NMPC_MARK(S_pf##i)
#define NMPC_SEC_KEEP(x) do { } while (0)
#define NMPC_PROBE_STATUS(s) do { } while (0)
#endif
#if defined(NMPC_PROF2) && NMPC_PROF2 == 2
#define NMPC_EVTICK(pe, i) do { if (pe) { __builtin_amdgcn_sched_barrier(0); const long long t_ = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xc07f); (pe)[i] += t_ - (pe)[7]; (pe)[7] = t_; __builtin_amdgcn_sched_barrier(0); } } while (0)
#define NMPC_EVAL_START() NMPC_STAMP(pe[7])
#define NMPC_EVAL_PE pe
#define NMPC_PROBE_STATUS(s) NMPC_PROBE_STATUS_(s, pe[0], pe[1], pe[2], pe[3], pe[4], pe[5], pe[6])
#else
#define NMPC_EVTICK(pe, i) NMPC_MARK(i)
#define NMPC_EVAL_START() do { } while (0)
#define NMPC_EVAL_PE nullptr
#ifdef NMPC_PROF2
#define NMPC_PROBE_STATUS(s) NMPC_PROBE_STATUS_(s, pf0, pf1, pf2, pf3, pf4, pf5, pf6)
#endif
#endif

// window statistics: NMPC_WIN_COUNT(k, hit) counts an attempt in counter k and, if hit, a failure in counter k + 1
#ifdef NMPC_WIN_STATS
__device__ unsigned long long nmpc_win_stats[4];       // evaluations that tried the window | of which fell back to the full scan | that tried the obstacle certificate | of which scanned
#define NMPC_WIN_COUNT(k, hit) do { if (lane == 0) { atomicAdd(&nmpc_win_stats[k], 1ull); if (hit) atomicAdd(&nmpc_win_stats[(k) + 1], 1ull); } } while (0)
#else
#define NMPC_WIN_COUNT(k, hit) do { } while (0)
#endif
#ifdef NMPC_BBCOUNT
__device__ __attribute__((used)) unsigned int nmpc_bbcnt[4096];
#endif
}  // namespace nmpc

// the readers of the instrumented builds; the product exports none of them
extern "C" {
#ifdef NMPC_TL
int nmpc_debug_timeline(long long *out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(nmpc::nmpc_tl), 64 * 16 * sizeof(long long)) == hipSuccess ? NMPC_OK : NMPC_ERR_HIP; }
#endif
#ifdef NMPC_BBCOUNT
int nmpc_debug_bbcount(unsigned int *out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(nmpc::nmpc_bbcnt), 4096 * sizeof(unsigned int));
    if (e == hipSuccess && reset) { static const unsigned int z[4096] = {0}; e = hipMemcpyToSymbol(HIP_SYMBOL(nmpc::nmpc_bbcnt), z, sizeof z); }
    return e == hipSuccess ? NMPC_OK : NMPC_ERR_HIP;
}
#endif
#ifdef NMPC_WIN_STATS
int nmpc_debug_win_stats(unsigned long long *out, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(nmpc::nmpc_win_stats), 4 * sizeof(unsigned long long));
    if (e == hipSuccess && reset) { const unsigned long long z[4] = {0, 0, 0, 0}; e = hipMemcpyToSymbol(HIP_SYMBOL(nmpc::nmpc_win_stats), z, sizeof z); }
    return e == hipSuccess ? NMPC_OK : NMPC_ERR_HIP;
}
#endif
}  // extern "C"
