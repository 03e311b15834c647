// Device side of the contract every persistent sweep lives by (decode_persistent.hip, train_persistent.hip, train_dual.hip,
// train_bwd_persistent.hip): write-through publishes, bounded waits on the arrival slots, and what a kernel does when a wait
// gives up.  The host side (option, first-use validation, error word) is SweepKernel in decoder_ws.h.
#pragma once
#include "common.h"

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64t;

// What a sweep needs to wait and to give up; one member of every kernel's argument struct, filled by sweep_sync_args (decoder_ws.h).
struct SweepSync {
  unsigned *cnt, *err;       // arrival slots (null: the decode kernel's granules carry their own tags), workspace error word
  unsigned* status;          // caller-owned sticky give-up flags (ZeggsDecCall.status), may be null
  unsigned spin;             // bound of every wait (option "persistent_spin")
  unsigned nap;              // s_sleep units between two polls (option "poll_sleep")
  unsigned stag;             // != 0: two staggered polls in flight (option "poll_stagger")
};

// A bounded wait gave up: the error word (read by the host after the first use on a process) and the caller's sticky status
// (read by the caller, and by zeggs_radam_step_guarded on the device, after every later use).  One thread per workgroup calls it;
// the NaN a kernel writes into what its consumers read first differs per kernel and stays in its epilogue.
__device__ __forceinline__ void sweep_gave_up(const SweepSync& y, unsigned bit) {
  atomicOr(y.err, 1u);
  if (y.status) atomicOr(y.status, bit);
}

__device__ __forceinline__ void stp(float* p, float v) {       // published: write-through
  __hip_atomic_store((gu32*)p, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// 16 bytes, write-through: one lane publishes four consecutive contraction indices (k % 4 == 0: in the forward the four hidden
// units of its workgroup) of one batch row = one float4 of the operand layout, a half-wave of batch rows 512 contiguous bytes --
// whole lines instead of byte-masked partial writes.
// NOTE the "memory" clobber is required (without it the results are corrupted), and with it the compiler drains every store it
// knows to be in flight (s_waitcnt vmcnt(0): about a microsecond) before this one: call stp4 BEFORE the plain stores of an
// epilogue, never after them.
__device__ __forceinline__ void stp4(float* p, f4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}

// Arrival slots: workgroup c publishes "I have finished phase instance p" by storing p + 1 into slot[c] (a write-through
// store, no read-modify-write to serialise); a consumer's polling wave loads all 256 slots with one 16-byte load per lane and
// waits until every slot has reached p + 1.  Epochs are monotonic and a workgroup can run at most one phase ahead of the
// slowest one, so one 1 KB array serves every phase.  Returns false on give-up.
// `mine` (per lane): this lane's four slots = the four workgroups that produce k-block `lane` of every exchanged vector (workgroup c
// owns hidden units 4c .. 4c+3 = a quarter of block c / 4) matter to the calling wave; a wave of the forward rollout waits for the
// producers of ITS k-blocks only (wave + 8 j: the lanes with lane % 8 == wave), the eight waves of a workgroup together for everybody.
__device__ __forceinline__ bool slots_wait(const unsigned* slots, unsigned expect, unsigned limit, bool mine = true, unsigned nap = 0) {
  const int lane = threadIdx.x & 63;
  const gu64t* q = (const gu64t*)(slots + 4 * lane);
  for (unsigned spins = 0;; ++spins) {
    const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool ok = !mine || ((unsigned)a >= expect && (unsigned)(a >> 32) >= expect && (unsigned)b >= expect && (unsigned)(b >> 32) >= expect);
    if (__all(ok)) return true;
    if (spins >= limit) return false;
    for (unsigned i = 0; i < nap; ++i) __builtin_amdgcn_s_sleep(1);
  }
}
// Two samples of the slots in flight, half a round trip apart (option "poll_stagger" = that half in s_sleep units, 0 = off): a
// producer's flag is seen by the first sample issued after it landed, i.e. after a quarter of a round trip on average instead of
// half of one (the round trip of a load that misses every cache is ~0.9 us: the dominant term of a hand-off).
__device__ __forceinline__ bool slots_wait2(const unsigned* slots, unsigned expect, unsigned limit, unsigned stagger) {
  const int lane = threadIdx.x & 63;
  const gu64t* q = (const gu64t*)(slots + 4 * lane);
  auto all_in = [&](unsigned long long a, unsigned long long b) {
    return __all((unsigned)a >= expect && (unsigned)(a >> 32) >= expect && (unsigned)b >= expect && (unsigned)(b >> 32) >= expect);
  };
  unsigned long long a0 = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  unsigned long long b0 = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (unsigned i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(1);
  for (unsigned spins = 0;; spins += 2) {
    const unsigned long long a1 = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b1 = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_in(a0, b0)) return true;
    a0 = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    b0 = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (all_in(a1, b1)) return true;
    if (spins >= limit) return false;
  }
}
