// The hand-managed device primitives of the gfx950 kernels, each defined ONCE: their correctness is a fact of the ISA, not of
// C++, so the hazard each one handles is explained here and nowhere else.  Included by pfn_internal.hpp (every unit sees it).
// tests/test_abi.py keeps it that way: no second copy of these instruction texts outside this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pfn {

// ------------------------------------------------------------------------------------- vector types
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ----------------------------------------------------------------------- float4 helpers, wave sums
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 fma4(float a, float4 x, float4 acc) {
    return make_float4(fmaf(a, x.x, acc.x), fmaf(a, x.y, acc.y), fmaf(a, x.z, acc.z), fmaf(a, x.w, acc.w));
}
__device__ __forceinline__ float4 mul4(float a, float4 x) { return make_float4(a * x.x, a * x.y, a * x.z, a * x.w); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
// (element-wise select: a ?: on the float4 struct goes through scratch)
__device__ __forceinline__ float4 sel4(bool k, float4 a, float4 b) { return make_float4(k ? a.x : b.x, k ? a.y : b.y, k ? a.z : b.z, k ? a.w : b.w); }
// ------------------------------------------------------------------------------ the ReLU and its gate
// ONE rule, the reference's (torch.relu / threshold_backward), in both directions and on every route: a unit is OFF iff its
// pre-activation compares <= 0.  A NaN compares false, so it is ON: the value stays NaN, the gate bit is 1 and the backward
// passes the incoming gradient through.  +Inf stays +Inf, -Inf gives 0.  The sign of a zero is not part of the contract (-0
// gives +0).  Never fmaxf(v, 0) or v > 0: both turn a NaN into "off, value 0" and bad data into plausible numbers.
__device__ __forceinline__ bool relu_on(float v) { return !(v <= 0.f); }
// (the value as ONE instruction, like the fmaxf it replaces: IEEE 754-2019 maximum propagates a NaN -- v_maximum3_f32 on gfx950;
//  as a compare + select the generic edge walks lost occupancy and 5-11 % of their time)
__device__ __forceinline__ float relu1(float v) { return __builtin_elementwise_maximum(v, 0.f); }
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }
// the gate applied: g where the unit whose pre-activation (or ReLU output: the same test) is `pre` is on, else 0
__device__ __forceinline__ float gate1(float pre, float g) { return pre <= 0.f ? 0.f : g; }
__device__ __forceinline__ float4 gate4(float4 pre, float4 g) { return make_float4(gate1(pre.x, g.x), gate1(pre.y, g.y), gate1(pre.z, g.z), gate1(pre.w, g.w)); }
// "ReLU or nothing" as one branch-free expression, x <= lo ? lo : x: lo = 0 is the ReLU, lo = -inf the identity for EVERY x (NaN
// and -Inf included)
__device__ __forceinline__ float clamp_lo(float x, float lo) { return __builtin_elementwise_maximum(x, lo); }
// sum over the 64 lanes of a wave as a FIXED xor butterfly (DPP / permute shuffles, no LDS, no barrier): every lane ends with the
// same, deterministic sum
__device__ __forceinline__ float4 wave_sum4(float4 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.x += __shfl_xor(v.x, off);
        v.y += __shfl_xor(v.y, off);
        v.z += __shfl_xor(v.z, off);
        v.w += __shfl_xor(v.w, off);
    }
    return v;
}

// ------------------------------------------------------------------------- barrier, LDS-DMA, drain
// Barrier that publishes LDS traffic only: __syncthreads() also waits (vmcnt(0)) until every outstanding GLOBAL access of the
// wave is acknowledged -- a round trip of 1-2 us under load at every barrier that follows output stores (phase timestamps: 1.5 us
// per hop of seg_lin_hops_kernel), and it pulls a prefetched next row group in front of the barrier.  Use only where no thread
// reads another thread's GLOBAL writes after the barrier.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// One 1 KiB LDS-DMA (64 lanes x 16 bytes; LDS destination = wave-uniform base + lane * 16, taken from m0: saved and restored
// around the copy, the s_nop is the wait state between a write of m0 and the LDS-DMA that reads it).
// Inline asm on purpose: while hipcc can see an LDS-DMA in flight it waits vmcnt(0) -- not a counted vmcnt -- for every
// ordinary load it later needs.  Hidden from the compiler, the DMA is waited for by hand (vmem_drain) before the barrier
// that publishes the copy; the compiler's own counted waits stay correct because VMEM returns in issue order.
__device__ __forceinline__ void dma_1k(const char* g, float* lds_dst) {
    const uint32_t m0v = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)((__attribute__((address_space(3))) float*)lds_dst));
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(g), "s"(m0v)
        : "memory");
}
// Drain of everything the wave has in flight in vector memory, hidden from hipcc's own wait-count bookkeeping: the hand-issued
// loads, DMAs and stores above and below are invisible to it, so it would not place this wait itself.  On gfx950 vmcnt counts
// stores too: behind a write-through store it means "the payload has left the XCD" (handoff_drained_publish below).
__device__ __forceinline__ void vmem_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ----------------------------------------------------------------------- the last-arriver hand-off
// Every block publishes a payload, takes a ticket on a counter and learns whether it is the LAST to arrive; the last one reads all
// payloads (in block order: reduce.hpp) and re-arms the counter with a plain store of 0.  Two flavours, both kept:
//   FENCED   plain payload stores by the thread that then calls handoff_fenced_publish (__threadfence, ACQ_REL ticket); every
//            thread of the last block calls handoff_fenced_consume (__threadfence) before it reads.  The language memory model
//            promises this form.  A __threadfence is an L2 write-back + L1 invalidate, ~3.5 us each on this multi-XCD part.
//   DRAINED  the payload is stored WRITE-THROUGH (agent_store), the stores are drained (vmem_drain), then a RELAXED ticket is
//            taken; the last block reads with agent_load (served by L2 / memory, never by its L1).  This is the "write-through
//            payload -> asm vmcnt(0) -> flag, agent-scope loads on the consumer" form MI355X_MICROARCH.md lists as valid ON gfx950
//            (vmcnt covers stores there; the language memory model does not promise it) -- hence the one target guard below, and
//            tests/test_gpu_parity.py::test_mse_loss_handoff_stress.  CONTRACT: the drain covers the calling WAVE only, so every
//            payload store must have been issued by the wave that calls handoff_drained_publish (any lane of it, any time before).
template <typename T>
__device__ __forceinline__ void agent_store(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T agent_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool handoff_fenced_publish(int* counter) {
    __threadfence();
    return __hip_atomic_fetch_add(counter, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
}
__device__ __forceinline__ void handoff_fenced_consume() { __threadfence(); }
__device__ __forceinline__ bool handoff_drained_publish(int* counter) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the drained last-arriver hand-off relies on gfx950 semantics (write-through stores drained by s_waitcnt vmcnt(0))"
#endif
    vmem_drain();
    return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
}

// --------------------------------------------------------------------------- hand-managed VMEM
// In the steady state of the GEMM kernels EVERY vector-memory instruction of a wave is inline asm, invisible to hipcc's waitcnt
// insertion, and every wait is a hand-counted `s_waitcnt vmcnt(N)` tied to the registers it protects:
//   * vload_x4 (16 bytes) / PFN_VLOAD_INTO (any width) write IN PLACE ("+v"): one 68-register fragment instead of the two sets
//     the register allocator keeps for a visible load (a spill anywhere in the flush costs a vmcnt(0) drain per reload --
//     measured 18 us/flush); a fresh output register ("=v": the value-returning forms) may be merged into its destination by a
//     copy that runs BEFORE the hidden load has landed, so a site keeps the form it has;
//   * a compiler-inserted wait would be vmcnt(0) (it cannot see the 17 younger prefetch loads) and drain the prefetch.
// VMEM returns in issue order and vmcnt counts loads and stores alike, so "wait until at most N younger ops are outstanding" is
// exact when N counts the ops issued after the one needed, and merely early when N is smaller.
// Address forms: `_addr` = a 64-bit per-lane pointer; otherwise a wave-uniform 64-bit base (SGPRs) + a 32-bit per-lane byte
// offset, which costs the VECTOR unit nothing.
// (the in-place load is a STATEMENT first: at gemm.hip's ring refill and gemm_nt.hip's row-scale load a function taking the
//  tied register by reference compiles to different code, like PFN_OPAQUE below; the 16-byte form is free as a function)
#define PFN_VLOAD_INTO(opcode, dst, sbase, voff) asm volatile(opcode " %0, %1, %2" : "+v"(dst) : "v"(voff), "s"(sbase) : "memory")
__device__ __forceinline__ void vload_x4(f32x4& dst, const char* sbase, uint32_t voff) {
    PFN_VLOAD_INTO("global_load_dwordx4", dst, sbase, voff);
}
__device__ __forceinline__ f32x4 vload_x4_addr(const float* p) {
    f32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ float vload_x1_addr(const float* p) {
    float r;
    asm volatile("global_load_dword %0, %1, off" : "=v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ float vload_x1_sv(const char* sbase, uint32_t voff) {
    float r;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(r) : "v"(voff), "s"(sbase) : "memory");
    return r;
}
template <int N>
__device__ __forceinline__ void wait_a(f32x4& v) {   // the register about to be consumed has landed: at most N younger ops in flight
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N));
}
// 16-byte stores.  The s_nop behind each is the ISA's "VMEM store wider than 64 bits -> VALU overwrites its data registers"
// hazard (2 wait states), which hipcc fills in for its own stores but cannot see inside inline asm (without it: intermittently
// wrong elements).
// WT = WRITE-THROUGH (sc1; hipcc has no 128-bit scoped store), for kernel OUTPUTS in global memory: a kernel's plain stores leave
// its output dirty in the XCD's L2 and the kernel boundary then waits for the write-back (MI355X_MICROARCH.md "boundary": + B /
// 6 TB/s behind B dirty bytes) -- ~1 us per launch of a chain whose every link is 10-30 us long; written through, the lines
// drain while the waves still run (gemm_nt back to back at 15,104 rows: 12.7 -> 11.9 / 18.9 -> 17.9 / 29.5 -> 28.7 us for 1 / 2 /
// 4 terms; `nt`: no change).  At large M it buys nothing and costs a few per cent: gemm_nt's CT = 2 kernels store plain.
template <bool WT = false>
__device__ __forceinline__ void vstore_x4(float* p, f32x4 v) {
    if (WT) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <bool WT = false>
__device__ __forceinline__ void vstore_x4_sv(const char* sbase, uint32_t voff, f32x4 v) {
    if (WT) asm volatile("global_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" : : "v"(voff), "v"(v), "s"(sbase) : "memory");
}
// the same store under a lane mask held in SGPRs -- exec narrowed and restored INSIDE the asm block: no branch, so the store stays
// in the basic block of the MFMAs it is interleaved with (gemm_nt_kernel's ILF); a lane whose mask bit is clear stores nothing.
// s_and_b64 overwrites SCC -- declared, so hipcc keeps no carry (the s_add_u32 / s_addc_u32 pair of the next store's 64-bit base)
// or compare result alive across the block; exec is back to its value when the block ends
__device__ __forceinline__ void vstore_x4_sv_masked(const char* sbase, uint32_t voff, f32x4 v, uint64_t mask) {
    uint64_t keep;
    asm volatile("s_mov_b64 %0, exec\n\ts_and_b64 exec, exec, %4\n\tglobal_store_dwordx4 %1, %2, %3\n\ts_mov_b64 exec, %0\n\ts_nop 1"
                 : "=&s"(keep)
                 : "v"(voff), "v"(v), "s"(sbase), "s"(mask)
                 : "memory", "scc");
}
// the write-through store of a float4 (the kernels outside gemm_nt: every one of their 16-byte output stores)
__device__ __forceinline__ void st4_wt(float* p, float4 v) { vstore_x4<true>(p, f32x4{v.x, v.y, v.z, v.w}); }

// ---------------------------------------------------------------- statements, not functions
// PFN_OPAQUE(x): an empty asm that "rewrites" x in its register.  hipcc can then neither hoist what is computed from x out of a
// loop (17 refill offsets -> 17 live VGPRs) nor sink what produced x into a later block.  A STATEMENT on purpose: as a function
// taking the tied register by reference it compiles to different code.  A site that ties several registers in ONE asm
// (edge.hip's big-graph hops) keeps its own spelling.
#define PFN_OPAQUE(x) asm volatile("" : "+v"(x))
// PFN_XDL_SETTLE("+v"(acc), ...): the last MFMA was issued a few instructions ago and its 16 passes are still writing the
// accumulators; hipcc's hazard recognizer does not look past the inline asm that closes a multiply, so the >= 18 wait states an
// XDL write needs before a VALU read are spent by hand (24 here; without them: intermittently stale accumulator rows).  The
// operands tie the accumulators the flush reads first, so nothing of it moves above the settle.
#define PFN_XDL_SETTLE(...) asm volatile("s_nop 15\n\ts_nop 7" : __VA_ARGS__)

}  // namespace pfn
