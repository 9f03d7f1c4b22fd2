// conv_dispatch.h -- routing of the conv / wgrad launches (C++ linkage, internal).
//
// A launch is DECIDED before it is made: a route function fills a Route -- which kernel instantiation, grid, block, dynamic LDS, the
// integer arguments the host computes -- and launches nothing; rd_route_launch() then launches exactly that.  The entry points
// (conv_api.hip) are validate -> route -> launch, and the queries (rd_conv_route, rd_conv_honours_src_out, the workspace sizes) read
// the same Route, so a query cannot disagree with a launch.  Each kernel file exposes "does this family take the launch, and if so
// fill the route"; the ORDER in which the families are asked is written once: conv_api.hip conv_route() and wgrad.hip rd_wgrad_route_plan().
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "../../include/ramdsir.h"
#include "bn_fin.h"

struct Route;
// One kernel instantiation.  RD_KERNEL makes the name, the address and the launch thunk from ONE source token, so a route's name
// cannot disagree with what is launched.
struct rd_kernel_t {
    const char* name;            // the instantiation as the table spells it
    const void* fn;              // its host stub
    void (*launch)(const Route&, const void* a, const void* b, hipStream_t);
    int attr;                    // hipFuncAttributeMaxDynamicSharedMemorySize to request: bytes, 0 = none, RD_ATTR_LDS = the launch's LDS size
    int attr_set;                // what has been requested so far (a larger launch raises it)
};
constexpr int RD_ATTR_LDS = -1;
#define RD_KERNEL(THUNK, ATTR, ...) { #__VA_ARGS__, reinterpret_cast<const void*>(&__VA_ARGS__), &THUNK<&__VA_ARGS__>, ATTR, 0 }

struct Route {
    rd_route_t v;                // the public image (ramdsir.h); v.kernel == k->name
    rd_kernel_t* k;
};
inline void rd_route_set(Route& r, rd_kernel_t& k, int gx, int gy, int gz, int block, size_t lds) {
    r = Route{};
    r.k = &k;
    r.v.kernel = k.name;
    r.v.grid[0] = gx; r.v.grid[1] = gy; r.v.grid[2] = gz;
    r.v.block = block;
    r.v.lds = (int)lds;
}
inline int rd_route_launch(const Route& r, const void* a, const void* b, hipStream_t st) {
    rd_kernel_t& k = *r.k;
    const int want = k.attr == RD_ATTR_LDS ? r.v.lds : k.attr;
    if (k.attr_set < want) {
        (void)hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, want);
        k.attr_set = want;
    }
    k.launch(r, a, b, st);
    return (int)hipGetLastError();
}
inline dim3 rd_route_grid(const Route& r) { return dim3(r.v.grid[0], r.v.grid[1], r.v.grid[2]); }
// launch thunks by kernel signature: (rd_conv_t, fin), (rd_conv_t, int, fin), (rd_wgrad_t, int, int, int, fin)
template <auto K> void rd_thunk_conv(const Route& r, const void* p, const void*, hipStream_t st) {
    rd_launch(K, rd_route_grid(r), dim3(r.v.block), (size_t)r.v.lds, st, *static_cast<const rd_conv_t*>(p), rdfin::current());
}
template <auto K> void rd_thunk_conv_i(const Route& r, const void* p, const void*, hipStream_t st) {
    rd_launch(K, rd_route_grid(r), dim3(r.v.block), (size_t)r.v.lds, st, *static_cast<const rd_conv_t*>(p), r.v.iarg[0], rdfin::current());
}
template <auto K> void rd_thunk_wgrad(const Route& r, const void* p, const void*, hipStream_t st) {
    rd_launch(K, rd_route_grid(r), dim3(r.v.block), (size_t)r.v.lds, st, *static_cast<const rd_wgrad_t*>(p), r.v.iarg[0], r.v.iarg[1], r.v.iarg[2],
              rdfin::current());
}

// ---- rd_conv: the families in the order conv_route() asks them.  A `bool` function returns false when its family does not take the launch.
bool rd_route_small_fwd(const rd_conv_t& p, int dtype, Route& r);      // conv_small_fwd.hip: bf16 3x3 forward, whole channel slots
void rd_route_small(const rd_conv_t& p, int dtype, Route& r);          // conv_small.hip: every other launch with one K chunk and one N block
bool rd_route_ws(const rd_conv_t& p, Route& r);                        // conv_pp.hip: conv_ws_kernel, the only kernel that writes rd_src_t.out
bool rd_route_pp(const rd_conv_t& p, Route& r);                        // conv_pp.hip: conv_pp_kernel (at most one tile per CU)
bool rd_route_pf_lean(const rd_conv_t& p, bool nb2, Route& r);         // conv_lean.hip: conv_pf_kernel with a register epilogue
bool rd_route_pf(const rd_conv_t& p, int dtype, bool nb2, Route& r);   // conv_big.hip: conv_pf_kernel, LDS-staged epilogue
void rd_route_conv_kernel(const rd_conv_t& p, int dtype, bool nb2, Route& r);   // conv_big.hip: the generic kernel takes what is left
bool rd_conv_nb2(const rd_conv_t& p, int dtype);                       // conv_big.hip: 64-channel output tiles?

// ---- rd_wgrad (wgrad.hip): out[0] the weight-gradient kernel, out[1] its split reduction; returns the number of launches
int rd_wgrad_route_plan(const rd_wgrad_t& p, int dtype, Route out[2]);
// wgrad_sym.hip: the 128 x 64-block kernel, grid (gx pixel splits, CoutPadW / 128, CinPadW / 64); partials in wgrad.hip's layout
void rd_route_wgrad_sym(const rd_wgrad_t& p, int gx, int CoutPadW, int CinPadW, Route& r);
// split reduction of per-workgroup weight-gradient sums partial[nsplit][taps][CoutPadW][CinPadW] -> dW; launched with the rd_wgrad_t
// that holds partial, dW and beta
void rd_route_wgrad_reduce(const float* partial, int nsplit, int taps, int Cout, int Cin, int CoutPadW, int CinPadW, Route& r);

// ---- fused dgrad + weight gradient of the small-channel 3x3 convs (conv_fused.hip): out[0] the kernel, out[1] the reduction
bool rd_bwd_fused_ok(const rd_conv_t& dgrad, const rd_wgrad_t& wgrad, int dtype);
void rd_bwd_fused_route(const rd_conv_t& dgrad, const rd_wgrad_t& wgrad, Route out[2]);

// Tiles per workgroup of the persistent small-channel kernels.  A launch runs in rounds of the resident workgroups (wgs_per_cu per
// compute unit); pick the count whose last round is (nearly) full -- e.g. 16 images x 650 tiles: 4 tiles / workgroup is 6 rounds x 4
// tile-times, 21 tiles / workgroup is 1 round x 21 -- charging `overhead` tile-times per workgroup (prologue, pipeline fill + drain).
// A limited launch (side lane: ramdsir.h cu_limit) must fit ONE round of its budget, however many tiles that takes.
inline int rd_tiles_per_wg(const rd_conv_t& p, int ntiles, int wgs_per_cu, double overhead, int cap, int round_to) {
    const bool limited = p.cu_limit > 0 && p.cu_limit < rd_num_cus();
    const long slots = (long)(limited ? p.cu_limit : rd_num_cus()) * wgs_per_cu;
    int tpw = 0;
    double best = 1e30;
    const int tmin = limited ? (int)(((long)ntiles * p.N + slots - 1) / slots) : 1;
    for (int t = tmin < 1 ? 1 : tmin; (t <= cap || limited) && t <= ntiles; ++t) {
        const long wgs = (long)((ntiles + t - 1) / t) * p.N;
        const double cost = (double)((wgs + slots - 1) / slots) * (t + overhead);
        if (cost < best - 1e-9) { best = cost; tpw = t; }
        if (limited) break;                                 // the smallest count that fits is the one
    }
    if (tpw <= 0) tpw = ntiles;
    return (tpw + round_to - 1) / round_to * round_to;
}

// Register ("lean") epilogues: accumulators leave as 16-byte NHWC vectors straight from registers (MFMA roles swapped:
// weights x pixels, rd_half_swap regroup) instead of through the LDS-staged epilogue of conv_epilogue.h.
// 0 = not eligible, 1 = forward, 2 = gradient with plain destinations only.  NT = output channels per workgroup.
inline int rd_conv_lean_mode(const rd_conv_t& p, int NT) {
    if (p.Cout != p.CoutPad || p.Cout % NT) return 0;
    if (p.emode == 0) return (((uintptr_t)p.out) & 15) == 0 ? 1 : 0;
    if (p.c_split % 16) return 0;
    bool any = false;
    for (int i = 0; i < 2; ++i) {
        const rd_dst_t& d = p.dst[i];
        if (i == 1 && p.c_split >= p.Cout) break;              // dst[1] unused
        if (d.kind == RD_DST_NONE) continue;
        any = true;
        const int width = i == 0 ? (p.c_split < p.Cout ? p.c_split : p.Cout) : p.Cout - p.c_split;
        if (d.kind != RD_DST_PLAIN || d.Cd % 8 || d.Cd < width || (((uintptr_t)d.g | (uintptr_t)d.z) & 15)) return 0;
        if (d.scale && (((uintptr_t)d.scale | (uintptr_t)d.shift) & 3)) return 0;
    }
    return any ? 2 : 0;
}
