// covt_wave.h -- wave64 primitives shared by the gfx950 kernels of libcovt (decode, assembly):
// wave-uniform reads, lane broadcast, DPP inclusive scan / max without LDS traffic.
#ifndef COVT_WAVE_H
#define COVT_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace covt {

// --------------------------------------------------------------------------------------------
// wave primitives
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return __lane_id(); }
__device__ __forceinline__ int32_t uni(int32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint32_t uniu(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ int64_t uni64(int64_t x) {
    const uint32_t lo = uniu((uint32_t)x), hi = uniu((uint32_t)((uint64_t)x >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint32_t lane_bcast(uint32_t x, int src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, src);
}
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// a DPP move of another lane's value; lanes without a source read `old` (64-bit: both halves)
template <int CTRL, int RMASK>
__device__ __forceinline__ uint32_t dpp_move(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, RMASK, 0xf, false);
}
template <int CTRL, int RMASK>
__device__ __forceinline__ uint64_t dpp_move(uint64_t old, uint64_t v) {
    const uint32_t lo = dpp_move<CTRL, RMASK>((uint32_t)old, (uint32_t)v);
    const uint32_t hi = dpp_move<CTRL, RMASK>((uint32_t)(old >> 32), (uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// The GFX9 wave64 scan sequence, no LDS traffic: row shifts within the 16-lane rows, then row broadcasts 15
// and 31 across them.  Step::step<CTRL, RMASK>(state...) is one step; after the six, lane l holds the
// combination of lanes 0 .. l (lane 63: of the whole wave).
template <class Step, class... S>
__device__ __forceinline__ void wave_dpp_seq(S&... s) {
    Step::template step<0x111, 0xf>(s...);  // row_shr:1
    Step::template step<0x112, 0xf>(s...);  // row_shr:2
    Step::template step<0x114, 0xf>(s...);  // row_shr:4
    Step::template step<0x118, 0xf>(s...);  // row_shr:8
    Step::template step<0x142, 0xa>(s...);  // row_bcast:15
    Step::template step<0x143, 0xc>(s...);  // row_bcast:31
}
// x := op(x, the moved x); lanes without a source combine with `old`, the operation's identity
template <class Op>
struct DppScanStep {
    template <int CTRL, int RMASK, class T>
    static __device__ __forceinline__ void step(T& x, const T& old) {
        x = Op::op(x, dpp_move<CTRL, RMASK>(old, x));
    }
};
// the inclusive scan of x over the 64 lanes under Op (uint32_t or uint64_t)
template <class Op, class T>
__device__ __forceinline__ T wave_scan(T x, T old = 0) {
    wave_dpp_seq<DppScanStep<Op>>(x, old);
    return x;
}

// unsigned add saturating at 0xffffffff (v_add_u32 with clamp)
__device__ __forceinline__ uint32_t add_sat(uint32_t a, uint32_t b) { return __builtin_elementwise_add_sat(a, b); }
struct OpAdd {
    template <class T>
    static __device__ __forceinline__ T op(T a, T b) { return a + b; }
    // (64-bit: two 32-bit adds, carry by hand)
    static __device__ __forceinline__ uint64_t op(uint64_t a, uint64_t b) {
        const uint32_t lo = (uint32_t)a + (uint32_t)b;
        const uint32_t hi = (uint32_t)(a >> 32) + (uint32_t)(b >> 32) + (lo < (uint32_t)a ? 1u : 0u);
        return ((uint64_t)hi << 32) | lo;
    }
};
struct OpAddSat {
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return add_sat(a, b); }
};
struct OpMax {
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b) { return max(a, b); }
};
struct OpOr {
    template <class T>
    static __device__ __forceinline__ T op(T a, T b) { return a | b; }
};

// inclusive prefix sum over the 64 lanes (wrapping uint32)
__device__ __forceinline__ uint32_t incl_scan(uint32_t x) { return wave_scan<OpAdd>(x); }
// inclusive prefix sum over the 64 lanes saturating at 0xffffffff: a sum that passes 2^32 - 1 stays there
// instead of wrapping, so a bound check on it cannot be fooled
__device__ __forceinline__ uint32_t incl_scan_sat(uint32_t x) { return wave_scan<OpAddSat>(x); }
// inclusive prefix sum of 64-bit values over the 64 lanes
__device__ __forceinline__ uint64_t incl_scan64(uint64_t x) { return wave_scan<OpAdd>(x); }
__device__ __forceinline__ uint64_t lane_bcast64(uint64_t x, int src) {
    return ((uint64_t)lane_bcast((uint32_t)(x >> 32), src) << 32) | lane_bcast((uint32_t)x, src);
}
// inclusive running maximum over the 64 lanes
__device__ __forceinline__ uint32_t incl_max_scan(uint32_t x) { return wave_scan<OpMax>(x); }
// maximum over the 64 lanes, returned uniform
__device__ __forceinline__ uint32_t wave_max(uint32_t x) { return lane_bcast(wave_scan<OpMax>(x), 63); }
// bitwise OR over the 64 lanes of a 64-bit value, returned uniform
__device__ __forceinline__ uint64_t wave_or64(uint64_t v) { return lane_bcast64(wave_scan<OpOr>(v), 63); }

// lane l + 1's value (lane 63: `tail`, which must be wave-uniform): DPP wave_shl:1, no LDS traffic.
// The DPP source lane has no successor for lane 63, which then keeps the `old` operand; keeping the
// select inside the DPP matters: a separate `l == 63 ? tail : dpp(x)` can be turned into an
// exec-masked branch, and a DPP move reading from a lane masked off returns the old value instead.
__device__ __forceinline__ uint32_t lane_next(uint32_t x, uint32_t tail = 0) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)tail, (int)x, 0x130, 0xf, 0xf, false);
}
// set bits of the 64-bit lane mask m below this lane (v_mbcnt_lo / _hi: two VALU, no 64-bit shifts)
__device__ __forceinline__ int32_t bits_below(uint64_t m) {
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// value of lane `src` (any lane index 0..63 per lane): ds_bpermute, no LDS allocation
__device__ __forceinline__ int32_t lane_get(int32_t x, int32_t src) {
    return __builtin_amdgcn_ds_bpermute(src << 2, x);
}
// f(src) once per lane whose pred is set, in lane order, the whole wave active in each call (src uniform): how
// a wave finishes, one after the other, the items that one lane each found too wide to take alone.  Every lane
// of the wave calls it.
template <class F>
__device__ __forceinline__ void wave_each(bool pred, F f) {
    for (uint64_t m = __ballot(pred); m; m &= m - 1) f(__ffsll((unsigned long long)m) - 1);
}

}  // namespace covt

#endif
