// xdt_args.h -- argument rules of aum_xdt_tm_fwd (include/aum_hip.h, ABI 9; delta_bias / flags: ABI 13), shared by the device library (gemm.hip) and the tests-only
// host build (tests/emu/aum_emu.cpp): no HIP dependency.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <initializer_list>

#include "../../include/aum_hip.h"

#define XDT_COLS 80          // columns of x_dbl = dt_rank + 2 d_state the kernels are built for (AuM-Base: 48 + 32)
#define XDT_COLS_SMALL 56    // ... and for AuM-Small's 24 + 32 (forward: any rank % 8 == 0; backward: the pairs (80, 48) and (56, 24) only)
#define XDT_COLS_TINY 48     // ... and, forward only, AuM-Tiny's 12 + 32 PADDED to three column fragments: [dt 12 | 4 zero columns | B 16 | C 16] with
                             // rank 16 -- the zero rows 12..15 of W_x and zero columns 12..15 of W_dt are the caller's (Mamba.stream_params)
#ifndef XDT_TOK_W
#define XDT_TOK_W 16         // tokens per wave
#endif
#define XDT_MAX_DIM 1536     // W_x passes through LDS in two K-halves of XDT_COLS rows: 80 x (768 x 2 + 16) bytes
// THE lists of what the kernels are instantiated for, each stated here alone: the checks below walk them, the dispatches (gemm.hip,
// aum_api_tm.inc) hand them to with_int, which refuses a value that is not listed
#define XDT_FWD_WIDTHS XDT_COLS, XDT_COLS_SMALL, XDT_COLS_TINY   // ncols of k_xdt_tm_fwd and k_stream_block
#define XDT_BWD_WIDTHS XDT_COLS, XDT_COLS_SMALL                  // ncols of k_xdt_tm_bwd
#define XDT_WAVES 8, 9, 10, 11, 12                               // waves (of XDT_TOK_W tokens) per workgroup: xdt_waves picks one from the token count
#define XDT_WAVES_MIN (std::min({XDT_WAVES}))

namespace aumx {
inline bool xdt_listed(int v, std::initializer_list<int> list) {
    for (int x : list)
        if (x == v) return true;
    return false;
}
// THE shapes of the forward pass (k_xdt_tm_fwd, and k_stream_block around the same body); aum_hip.xdt_tm_supported states the same rule.
//   ncols: a width the body is instantiated for.
//   dim % 128: W_x passes through LDS in two K-halves walked in steps of 64 columns, so a half is a whole number of steps.  Everything
//     else the body does with dim is implied: the conv_out prefetch ring runs over dim / 64 steps (an even count: it ends after two or
//     after four steps of a round), a W_dt channel half is dim / 2 channels = dim / 64 pairs of 32, its bias is staged as dim / 8 float4.
inline bool xdt_fwd_shape_ok(int ncols, int dim) {
    return xdt_listed(ncols, {XDT_FWD_WIDTHS}) && dim > 0 && dim % 128 == 0 && dim <= XDT_MAX_DIM;
}
inline int xdt_check(const AumXdtArgs* p) {
    if (!p || !p->u || !p->wx || !p->wdt || !p->x_dbl || !p->delta) return AUM_E_NULL;
    const AumXdtArgs& g = *p;
    if (g.ntok <= 0 || g.dim <= 0 || g.rank <= 0 || g.ncols <= 0 || g.ldu < g.dim || g.ldwx < g.dim || g.ldwdt < g.rank || g.ldx < g.ncols ||
        g.ldd < g.dim)
        return AUM_E_SHAPE;
    if (g.dtype != AUM_BF16 && g.dtype != AUM_F16) return AUM_E_DTYPE;
    if (!xdt_fwd_shape_ok(g.ncols, g.dim) || g.rank % 8 || g.rank > 64 || g.rank > g.ncols) return AUM_E_UNSUPPORTED;
    if (g.ldu % 8 || g.ldwx % 8 || g.ldwdt % 8 || g.ldx % 8 || g.ldd % 8) return AUM_E_UNSUPPORTED;
    if (((uintptr_t)g.u | (uintptr_t)g.wx | (uintptr_t)g.wdt | (uintptr_t)g.x_dbl | (uintptr_t)g.delta) & 15u) return AUM_E_UNSUPPORTED;
    // the bias is staged 16 bytes at a time and only ever added together with the softplus
    if ((g.flags & ~AUM_XDT_DELTA_SOFTPLUS) || (g.delta_bias && !(g.flags & AUM_XDT_DELTA_SOFTPLUS)) || ((uintptr_t)g.delta_bias & 15u))
        return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
inline int xdt_bwd_check(const AumXdtBwdArgs* p) {
    if (!p || !p->ddelta || !p->dbc || !p->wdt_t || !p->wx_t || !p->du || !p->dx_dbl) return AUM_E_NULL;
    const AumXdtBwdArgs& g = *p;
    if (g.ntok <= 0 || g.dim <= 0 || g.rank <= 0 || g.ncols <= 0 || g.ldd < g.dim || g.ldu < g.dim || g.ldwdt < g.dim || g.ldwx < g.ncols ||
        g.ldx < g.ncols || g.lddbc < g.ncols - g.rank)
        return AUM_E_SHAPE;
    if (g.dtype != AUM_BF16 && g.dtype != AUM_F16) return AUM_E_DTYPE;
    if (!xdt_listed(g.ncols, {XDT_BWD_WIDTHS}) || g.rank != g.ncols - 32 || g.dim % 256 || g.dim > XDT_MAX_DIM) return AUM_E_UNSUPPORTED;
    if (g.ldd % 8 || g.ldu % 8 || g.ldwdt % 8 || g.ldwx % 8 || g.ldx % 8 || g.lddbc % 4) return AUM_E_UNSUPPORTED;
    if (((uintptr_t)g.ddelta | (uintptr_t)g.dbc | (uintptr_t)g.wdt_t | (uintptr_t)g.wx_t | (uintptr_t)g.du | (uintptr_t)g.dx_dbl) & 15u)
        return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
// waves per workgroup for `ntok` tokens on `ncu` CUs (one workgroup per CU at a time): the count of XDT_WAVES whose launch takes the fewest
// wave-rounds, rounds x waves -- 2052 fragments on 256 CUs: 8 waves = 257 workgroups = 2 rounds (16), 9 waves = 228 = 1 round (9)
inline int xdt_waves(int64_t ntok, int ncu) {
    const int64_t frags = (ntok + XDT_TOK_W - 1) / XDT_TOK_W;
    int best = 0;
    int64_t best_cost = -1;
    for (int nw : {XDT_WAVES}) {
        const int64_t wgs = (frags + nw - 1) / nw, cost = (wgs + ncu - 1) / ncu * nw;
        if (best_cost < 0 || cost < best_cost) {
            best = nw;
            best_cost = cost;
        }
    }
    return best;
}
}  // namespace aumx
