// covt_coop.h -- the thread group that works on one geometry column and its scans, shared by the
// assembly passes (covt_assemble.hip) and the geometry products: a wave (NW = 1) or a whole workgroup of
// NW waves, IPL items of a step per thread, saturating exclusive scans over a step (excl_scan4) and over a
// column's items step by step (StepScan); and the global-address-space pointer types of the device code.
#ifndef COVT_COOP_H
#define COVT_COOP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "covt_wave.h"

namespace covt {

// Pointer types of the device code's global loads and stores: g_* is const, gw_* writable; a trailing u is an
// alignment of 1 (gfx950 runs with unaligned access mode on: such an access stays one instruction).
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint64_t u64u __attribute__((aligned(1)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
typedef double f64x2u __attribute__((ext_vector_type(2), aligned(1)));
typedef __attribute__((address_space(1))) const uint8_t g_u8;
typedef __attribute__((address_space(1))) const int32_t g_i32;
typedef __attribute__((address_space(1))) const uint32_t g_u32;
typedef __attribute__((address_space(1))) const int64_t g_i64;
typedef __attribute__((address_space(1))) const uint64_t g_u64;
typedef __attribute__((address_space(1))) const double g_f64;
typedef __attribute__((address_space(1))) const i32x4 g_i32x4;
typedef __attribute__((address_space(1))) const u32x4 g_u32x4;
typedef __attribute__((address_space(1))) const u32x4u g_u32x4u;
typedef __attribute__((address_space(1))) uint8_t gw_u8;
typedef __attribute__((address_space(1))) int32_t gw_i32;
typedef __attribute__((address_space(1))) uint32_t gw_u32;
typedef __attribute__((address_space(1))) int64_t gw_i64;
typedef __attribute__((address_space(1))) uint64_t gw_u64;
typedef __attribute__((address_space(1))) double gw_f64;
typedef __attribute__((address_space(1))) u32x4 gw_u32x4;
typedef __attribute__((address_space(1))) u16u gw_u16u;
typedef __attribute__((address_space(1))) u32u gw_u32u;
typedef __attribute__((address_space(1))) u64u gw_u64u;
typedef __attribute__((address_space(1))) f64x2u gw_f64x2u;

template <int NW, int IPL = 4>
struct __attribute__((aligned(16))) AsmSmemT {
    int32_t slot[IPL * 64 * NW];  // expansion: segment-end marks of the current step
    int32_t ends[IPL * 64 * NW];  // expansion: the step's segment ends
    uint32_t red[2][NW];          // cooperative scans / reductions: per-wave totals (two buffers)
};

// The threads assembling one column: a wave (NW = 1: lane_id, wave primitives, no barrier) or a whole
// workgroup of NW waves (thread index, per-wave partials through LDS and workgroup barriers).  Items
// of a step: IPL consecutive per thread, K = 64 IPL NW per step.
template <int NW, int IPL = 4>
struct Coop {
    static constexpr int K = IPL * 64 * NW;
    __device__ __forceinline__ static int tid() { return NW == 1 ? lane_id() : (int)threadIdx.x; }
    __device__ __forceinline__ static int wid() { return NW == 1 ? 0 : (int)(threadIdx.x >> 6); }
    // exclusive prefix of a per-thread value over the group (wave inclusive `inc` given, saturating),
    // group total.  Sums saturate at 0xffffffff: every count is checked against a capacity below 2^31, so
    // a saturated total fails the check, where a wrapped one could pass it (a 4096-item cooperative step
    // of clamped counts can reach 2^32).  A saturated prefix is only ever stored for a failing column.
    template <int I>
    __device__ __forceinline__ static uint32_t group_prefix(AsmSmemT<NW, I>& sm, uint32_t inc, uint32_t own,
                                                           uint32_t& tot, int buf) {
        if (NW == 1) {
            tot = lane_bcast(inc, 63);
            return inc - own;
        }
        if (lane_id() == 63) sm.red[buf][wid()] = inc;
        __syncthreads();
        uint32_t pre = 0, all = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t t = sm.red[buf][i];
            pre = add_sat(pre, i < wid() ? t : 0u);
            all = add_sat(all, t);
        }
        tot = all;
        return add_sat(pre, inc - own);
    }
};

// exclusive scan of the step's items held IPL per thread (items IPL t .. IPL t + IPL - 1); `tot` gets the
// uniform total.  Cooperative groups alternate the two partial buffers (each buffer is rewritten only after
// a barrier that follows every read of its previous contents).
template <int NW, int IPL>
__device__ __forceinline__ void excl_scan4(AsmSmemT<NW, IPL>& sm, int& buf, const uint32_t (&x)[IPL], uint32_t (&ex)[IPL],
                                           uint32_t& tot) {
    if (NW == 1) {  // lane-major items: a wave scan per row of 64, rows carried in order
        uint32_t carry = 0;
#pragma unroll
        for (int k = 0; k < IPL; ++k) {
            const uint32_t inc = incl_scan_sat(x[k]);
            ex[k] = add_sat(carry, inc - x[k]);
            carry = add_sat(carry, lane_bcast(inc, 63));
        }
        tot = carry;
        buf ^= 1;
        return;
    }
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < IPL; ++k) s = add_sat(s, x[k]);  // saturating: see group_prefix
    const uint32_t inc = incl_scan_sat(s);
    uint32_t run = Coop<NW, IPL>::group_prefix(sm, inc, s, tot, buf);
    buf ^= 1;
#pragma unroll
    for (int k = 0; k < IPL; ++k) {
        ex[k] = run;
        run = add_sat(run, x[k]);
    }
}

// The exclusive scan of n items in steps of K by the group, the shape of every per-column offsets scan: item i's
// value load(i) -> store(i, its saturated exclusive prefix), i < n; returns the saturated total (uniform).  Every
// thread of the group calls run() with the same n, so all of them reach excl_scan4's barriers the same number
// of times.  One StepScan serves all the scans of a column in turn: `buf` goes on alternating across them.
template <int NW, int IPL>
struct StepScan {
    AsmSmemT<NW, IPL>& sm;
    int buf = 0;

    template <class Load, class Store>
    __device__ __forceinline__ uint32_t run(int32_t n, Load load, Store store) {
        const int l = Coop<NW, IPL>::tid();
        auto ioff = [&](int k) { return NW == 1 ? 64 * k + l : IPL * l + k; };  // the step's k-th item of this thread
        uint32_t base = 0;
        for (int32_t i0 = 0; i0 < n; i0 += Coop<NW, IPL>::K) {
            uint32_t x[IPL], ex[IPL], tot;
#pragma unroll
            for (int k = 0; k < IPL; ++k) {
                const int32_t i = i0 + ioff(k);
                x[k] = i < n ? load(i) : 0u;
            }
            excl_scan4(sm, buf, x, ex, tot);
#pragma unroll
            for (int k = 0; k < IPL; ++k) {
                const int32_t i = i0 + ioff(k);
                if (i < n) store(i, add_sat(base, ex[k]));
            }
            base = add_sat(base, tot);
        }
        return base;
    }
    // the total alone
    template <class Load>
    __device__ __forceinline__ uint32_t sum(int32_t n, Load load) {
        return run(n, load, [](int32_t, uint32_t) {});
    }
    // v[0 .. n) -> its exclusive scan in place (the per-chunk totals of a count pass -> the chunks' bases)
    __device__ __forceinline__ uint32_t in_place(uint32_t* v, int32_t n) {
        return run(n, [&](int32_t i) { return ((g_u32*)v)[i]; }, [&](int32_t i, uint32_t e) { ((gw_u32*)v)[i] = e; });
    }
};

}  // namespace covt

#endif
