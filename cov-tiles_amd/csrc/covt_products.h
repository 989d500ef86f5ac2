// covt_products.h -- the per-column products of a plan: what is computed once per geometry column (WKB, bounding
// boxes, measures, select, simplify, MVT).  A product is the trait struct of its plan header (Info, Desc, Res,
// layout, fill); this file lists them and holds the one writer of a column's record and descriptor, shared by the
// host plan (covt_host.cpp) and the device plan (covt_plan_device.hip).  Plain C++17, no HIP calls:
// tests/product_records/product_records_check.cc runs it on the CPU under sanitizers.
#ifndef COVT_PRODUCTS_H
#define COVT_PRODUCTS_H

#include <stdint.h>

#include <tuple>

#include "covt.h"
#include "covt_wkb_plan.h"
#include "covt_bbox_plan.h"
#include "covt_measures_plan.h"
#include "covt_select_plan.h"
#include "covt_simplify_plan.h"
#include "covt_mvt_plan.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COVT_PRODUCTS_HD __host__ __device__
#else
#define COVT_PRODUCTS_HD
#endif

template <class... P>
struct ProductList {
    // a plan's state: one S<P> per product, reached with std::get<S<P>>
    template <template <class> class S>
    using Each = std::tuple<S<P>...>;
    // f(P{}) for every product, in list order
    template <class F>
    static void for_each(F&& f) { (f(P{}), ...); }
};
// The list, in the order both plans build the products and the device plan lays them out in its geometry arena.
using Products = ProductList<WkbProduct, BboxProduct, MeasuresProduct, SelectProduct, SimplifyProduct, MvtProduct>;

// Product P's record `info` of geometry column g, whose slice starts at `off` (16-byte aligned), and its
// descriptor at the geometry descriptor's row of `desc`; returns the offset after the slice.
template <class P>
COVT_PRODUCTS_HD inline int64_t product_record(const covt_geom_info& g, int64_t off, typename P::Info& info,
                                               typename P::Desc* desc) {
    typename P::Desc d{};
    off = P::layout(g, off, d);
    typename P::Info r{};
    r.tile = g.tile;
    r.layer = g.layer;
    r.n_features = d.n_features;
    r.desc_index = g.desc_index;
    r.flags = d.flags;
    P::fill(r, d);
    info = r;
    desc[g.desc_index] = d;
    return off;
}

#endif
