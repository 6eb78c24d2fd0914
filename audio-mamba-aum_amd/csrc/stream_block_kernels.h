// stream_block_kernels.h -- the recurrent middle of the causal block on packed streaming sessions in ONE launch (include/aum_hip.h:
// aum_stream_block_tm): causal conv from the carried window -> x_proj / dt_proj (softplus once) -> selective scan from the carried state.
//
// At hop sizes (8 .. 32 tokens per session) the three launches this replaces -- k_convt_chunk_var, k_xdt_tm_fwd, k_stream_scan_chunk_var --
// are bound by being three launches: the projections already run as one workgroup, and spreading a session's conv and scan over a few
// dozen waves buys nothing when the next launch cannot start sooner (profiles/r07_stream_hop.txt).  Here ONE workgroup of SB_NW waves
// owns a session and walks its rows through three phases:
//   1. conv:  the waves share out the session's channel blocks, each a convc_unit (stream_tm_kernels.h) -> xc
//   2. x/dt:  the body of k_xdt_tm_fwd (xdt_fwd_body.inc) on the session's rows as workgroup 0 of a stream of `len` tokens: W_x and W_dt through LDS,
//             the products on the matrix pipe (v_mfma_f32_16x16x32), SB_NW * 16 tokens at most -> x_dbl, delta.  NC = 80 / 56 / 48 columns
//             (AuM-Base / -Small / -Tiny's padded rows, xdt_args.h); B | C sit at x_dbl + rank at every width
//   3. scan:  the waves share out the session's groups of 64 channels, each a scanc_unit (delta activated, z gate) -> y
// The step routines are the ones the three kernels run, so y and both cache rows are bit for bit theirs (every step is the same
// instruction sequence on the same values: -ffp-contract=off, and an MFMA column -- a token -- does not depend on its neighbours).
//
// xc, delta and x_dbl cross the phases through the caller's scratch: (total, dim), (total, dim), (total, ncols) rows of which this
// workgroup reads and writes the rows of its own session only.  A phase is separated from the next by __syncthreads(), whose
// workgroup-scope fence orders the global stores of one wave before the loads of another wave of the same workgroup (one CU, one vector
// L1).  There is NO ordering between workgroups: no grid sync, no flags, no atomics -- sessions are independent.
// (The tiles are kept out of LDS on purpose: the projection phase already holds 143 KB of the 160 KB for the weight slab, and
// SB_MAX_T x 1536 channels x 2 tensors is 768 KB.  At hop sizes the rows are a few dozen KB that never leave L2.)
#pragma once
#include "stream_tm_kernels.h"
#ifndef AUM_EMU
#include "xdt_kernels.h"          // device only (MFMA): the lane-array test build composes the three host entry points instead
#else
#include "xdt_args.h"
#endif

namespace aum {

constexpr int SB_NW = 8;                              // waves per workgroup: what k_xdt_tm_fwd runs with at these token counts
constexpr int SB_MAX_T = SB_NW * XDT_TOK_W;           // tokens per session and call (STREAM_BLOCK_MAX_T = 128)

// scratch rows (elements of the 16-bit dtype): xc at 0, delta behind it, x_dbl behind that
struct SbScratch { int64_t xc, delta, x_dbl, total; };
AUM_HOSTDEV SbScratch sb_scratch(int64_t total, int dim, int ncols) {
    SbScratch s;
    s.xc = 0;
    s.delta = total * dim;
    s.x_dbl = 2 * total * dim;
    s.total = s.x_dbl + total * ncols;
    return s;
}

#ifndef AUM_EMU
// The arguments, read where they are used.  A phase that held `a` by value would keep every field it shares with a later phase in a scalar
// register across the phases between them, and scanc_unit alone takes nearly the whole scalar file (k_stream_scan_chunk_var: 104 of 104):
// the compiler then parks scalars in vector lanes.  Instead every phase -- every unit of the conv and of the scan -- reads its fields
// from the kernel argument segment again (the struct is the kernel's only argument, so it sits at offset 0 of the segment; scalar loads
// that hit the scalar cache), behind an empty asm that keeps the compiler from merging those loads with an earlier phase's.  What
// crosses a phase is the session (r0, len, row) and the wave's index.
AUM_DEV const AumStreamBlockArgs& sb_args() {
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const AumStreamBlockArgs*)p;
}
template <class T> AUM_DEV T* sb_rows(const AumStreamBlockArgs& a, int64_t at, int r0, int pitch) {
    return static_cast<T*>(a.scratch) + at + (int64_t)r0 * pitch;
}

// PEEK (AUM_STREAM_PEEK_LAST): the units close the caches one row early (stream_tm_kernels.h); the projections take every row
template <class T, bool BF16, int KS, int NC, bool PEEK = false>
__global__ __launch_bounds__(SB_NW * 64, 1) void k_stream_block(AumStreamBlockArgs) {
    __shared__ __attribute__((aligned(16))) char lds[aumx::lds_bytes(XDT_MAX_DIM, SB_NW)];
    int r0, len, row, ncb, ngrp;
    {
        const AumStreamBlockArgs& a = sb_args();
        // the whole workgroup takes the same way out: no barrier is left behind
        if (!stream_seq(a.cu_seqlens, a.state_indices, (int)blockIdx.x, a.total, a.nrows, r0, len, row) || len > a.max_len) return;
        ncb = convt_cblocks<T, false>(a.dim);
        ngrp = a.dim / WAVE;
    }
    // ---- 1. conv ------------------------------------------------------------------------------------------------------------
    for (int cb = wave_in_wg(); cb < ncb; cb += SB_NW) {
        const AumStreamBlockArgs& a = sb_args();
        const SbScratch so = sb_scratch(a.total, a.dim, a.ncols);
        const ConvcOps o = {a.conv_weight, a.conv_bias, a.x_ts, (int64_t)a.dim, a.dim, a.width};
        convc_unit<T, true, PEEK>(o, row_ptr<T>(a.x, (int64_t)r0 * a.x_ts), sb_rows<T>(a, so.xc, r0, a.dim), a.conv_state + (int64_t)row * a.dim * a.width,
                                  len, cb, !(a.flags & AUM_STREAM_NO_COMMIT));
    }
    __syncthreads();
    // ---- 2. x_proj, dt_proj, softplus ---------------------------------------------------------------------------------------------
    {
        using namespace aumx;
        constexpr int NW = SB_NW;
        constexpr bool SOFTPLUS = true;
        AumXdtArgs g;
        {
            const AumStreamBlockArgs& a = sb_args();
            const SbScratch so = sb_scratch(a.total, a.dim, a.ncols);
            g.u = sb_rows<T>(a, so.xc, r0, a.dim); g.wx = a.wx; g.wdt = a.wdt;
            g.x_dbl = sb_rows<T>(a, so.x_dbl, r0, a.ncols); g.delta = sb_rows<T>(a, so.delta, r0, a.dim);
            g.ntok = len;
            g.dim = a.dim; g.rank = a.rank; g.ncols = a.ncols;
            g.ldu = a.dim; g.ldwx = a.ldwx; g.ldwdt = a.ldwdt; g.ldx = a.ncols; g.ldd = a.dim;
            g.dtype = a.dtype;
            g.delta_bias = a.delta_bias;
            g.flags = AUM_XDT_DELTA_SOFTPLUS;
        }
#define XDT_BODY_WG 0
#include "xdt_fwd_body.inc"
#undef XDT_BODY_WG
    }
    __syncthreads();
    // ---- 3. scan ------------------------------------------------------------------------------------------------------------
    for (int grp = wave_in_wg(); grp < ngrp; grp += SB_NW) {
        const AumStreamBlockArgs& a = sb_args();
        const SbScratch so = sb_scratch(a.total, a.dim, a.ncols);
        const T *xc = sb_rows<T>(a, so.xc, r0, a.dim), *x_dbl = sb_rows<T>(a, so.x_dbl, r0, a.ncols);
        const ScancOps o = {a.A, a.D, nullptr, (int64_t)a.dim, (int64_t)a.dim, a.z_ts, (int64_t)a.ncols, (int64_t)a.ncols, a.y_ts};
        const ScancSeq<T> q = {xc, sb_rows<T>(a, so.delta, r0, a.dim), row_ptr<T>(a.z, (int64_t)r0 * a.z_ts), x_dbl + a.rank, x_dbl + a.rank + SCANT_N,
                               row_ptr<T>(a.y, (int64_t)r0 * a.y_ts), a.state + (int64_t)row * a.dim * SCANT_N, len};
        scanc_unit<T, false, true, PEEK>(o, q, grp * WAVE, !(a.flags & AUM_STREAM_NO_COMMIT));
    }
}
#endif

}  // namespace aum
