// stream_stack_kernels.h -- the two skinny projections of a streaming hop (include/aum_hip.h: aum_stream_in_tm, aum_stream_out_tm), the
// launches aum_stream_layers enqueues around k_stream_block:
//   k_stream_in    residual_out = hidden (+ residual_in);  normed = rmsnorm(residual_out) * w_norm;  xz = normed . W_in^T
//   k_stream_out   out = y . W_out^T
// M is the rows of a hop (8 .. 150), so both stream their weight matrix once and are bound by how soon the bytes arrive, not by the
// matrix pipe.  A workgroup of SS_NW waves owns NF fragments of 16 OUTPUT COLUMNS and keeps their weight rows in registers for the whole
// launch: wave w holds the K-steps of 32 with step % SS_NW == w (lane (kg, rho): row rho of the fragment, k = 32 step + 8 kg .. + 7, one
// 16-byte load).  The rows are walked in tiles of 16 tokens: weights are the MFMA's A operand, the 16 tokens its B operand
// (v_mfma_f32_16x16x32: lane (kg, rho) holds token rho's k = 32 step + 8 kg .. + 7), so an accumulator column is ONE token and a token's
// sums never meet another token's.  Every wave chains its own steps in ascending order into one fp32 accumulator, the SS_NW partial
// accumulators cross LDS, and wave f adds them in wave order ((p0 + p1) + p2) + p3 for fragment f, rounds once and stores.  The order
// depends on K alone: not on total, not on the row's place in the pack, not on its neighbours.
// k_stream_in's B operand is the normed tile in LDS: for every tile the waves share out its 16 rows and run rmsnorm_fwd_vec
// (conv_norm_kernels.h, the row routine of aum_rmsnorm_fwd) with the tile as its y -- the same statements on the same values, so
// residual_out and the rounded row are aum_rmsnorm_fwd's bits.  Every workgroup recomputes the prologue (total x d_model values from L2,
// comparable to its own weight slab at hop sizes); workgroup 0 alone hands the routine a residual_out.  residual_in is read by all
// workgroups at times nothing orders: it must not be residual_out (the host check refuses it).
// Bounds: weight rows col0 + 16 f + rho < N because the grid is exactly N / (16 NF) and N % (16 NF) == 0 at the built widths; k < K by
// the step guard; rows t0 + rho < total guard every load of a token row and every store.
// No workgroup waits for another: no grid sync, no flags, no atomics, no partial sums through memory.
// The lane-array build has no matrix pipe: plain host loops over (row, column) with an fp32 accumulator and ascending k, the norm
// prologue through the lane-array form of the same row routine.
#pragma once
#include <stdint.h>
#include "../../include/aum_hip.h"
#include "wave.h"
#include "conv_norm_kernels.h"
#ifndef AUM_EMU
#include "xdt_kernels.h"          // aumx::mfma, pack2 and the vector types
#else
#include <vector>
#endif

namespace aum {

constexpr int SS_NW = 4;              // waves per workgroup: the K-steps go round robin over them
constexpr int SS_TILE = 16;           // token rows per MFMA tile
constexpr int SS_IN_NF = 2;           // fragments of 16 output columns per workgroup: in_proj (the norm prologue is shared by 32 columns)
constexpr int SS_OUT_NF = 1;          // ... out_proj

// the widths the kernels are instantiated for: (d_model, dim) = (192, 384), (384, 768), (768, 1536)
AUM_HOSTDEV bool ss_widths_ok(int d_model, int dim) { return (d_model == 192 || d_model == 384 || d_model == 768) && dim == 2 * d_model; }
static inline bool ss_dtype16(int dtype) { return dtype == AUM_BF16 || dtype == AUM_F16; }

// ---- operand checks (aum_hip.stream_in_args_ok / stream_out_args_ok mirror them rule for rule) ------------------------------------------
static inline int ss_in_check(const AumStreamInArgs* a) {
    if (!a || !a->hidden || !a->norm_weight || !a->w_in || !a->residual_out || !a->xz) return AUM_E_NULL;
    if (a->total <= 0 || a->d_model <= 0 || a->dim <= 0) return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2 || a->dtype == AUM_F32) return AUM_E_DTYPE;
    if (!ss_widths_ok(a->d_model, a->dim)) return AUM_E_UNSUPPORTED;
    if (a->hidden_ts < a->d_model || a->xz_ts < 2 * (int64_t)a->dim || a->ldw < a->d_model || ((a->hidden_ts | a->xz_ts | a->ldw) & 7)) return AUM_E_UNSUPPORTED;
    const uintptr_t ptrs = (uintptr_t)a->hidden | (uintptr_t)a->residual_in | (uintptr_t)a->norm_weight | (uintptr_t)a->w_in | (uintptr_t)a->residual_out |
                           (uintptr_t)a->xz;
    if (ptrs & 15) return AUM_E_UNSUPPORTED;
    if (a->residual_in == a->residual_out) return AUM_E_UNSUPPORTED;      // read by every workgroup while workgroup 0 writes
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if ((int64_t)a->total * (a->hidden_ts > a->xz_ts ? a->hidden_ts : a->xz_ts) * 2 > lim) return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
static inline int ss_out_check(const AumStreamOutArgs* a) {
    if (!a || !a->y || !a->w_out || !a->out) return AUM_E_NULL;
    if (a->total <= 0 || a->d_model <= 0 || a->dim <= 0) return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2 || a->dtype == AUM_F32) return AUM_E_DTYPE;
    if (!ss_widths_ok(a->d_model, a->dim)) return AUM_E_UNSUPPORTED;
    if (a->y_ts < a->dim || a->out_ts < a->d_model || a->ldw < a->dim || ((a->y_ts | a->out_ts | a->ldw) & 7)) return AUM_E_UNSUPPORTED;
    if (((uintptr_t)a->y | (uintptr_t)a->w_out | (uintptr_t)a->out) & 15) return AUM_E_UNSUPPORTED;
    if (a->y == a->out) return AUM_E_UNSUPPORTED;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if ((int64_t)a->total * (a->y_ts > a->out_ts ? a->y_ts : a->out_ts) * 2 > lim) return AUM_E_UNSUPPORTED;
    return AUM_OK;
}

// the norm prologue of rows [t0, t0 + SS_TILE) as aum_rmsnorm_fwd sees one row: y = the tile (pitch y_pitch elements)
template <class T> AUM_HOSTDEV AumNormArgs ss_norm_args(const AumStreamInArgs& a, int64_t t0, void* tile, int64_t y_pitch, bool write_residual) {
    AumNormArgs p = {};
    p.x = static_cast<const T*>(a.hidden) + t0 * a.hidden_ts;
    p.residual = a.residual_in ? a.residual_in + t0 * a.d_model : nullptr;
    p.weight = a.norm_weight;
    p.y = tile;
    p.residual_out = write_residual ? a.residual_out + t0 * a.d_model : nullptr;
    p.row_stride_x = a.hidden_ts; p.row_stride_res = a.d_model; p.row_stride_y = y_pitch; p.row_stride_res_out = a.d_model;
    p.eps = a.eps;
    p.rows = SS_TILE; p.cols = a.d_model;
    return p;
}

#ifdef AUM_EMU
// ---- lane-array build: host loops ------------------------------------------------------------------------------------------------------
template <class T> static inline void ss_dot_row(const T* arow, const T* w, int64_t ldw, int n, int k, T* orow) {
    for (int c = 0; c < n; ++c) {
        float acc = 0.f;
        for (int i = 0; i < k; ++i) acc = acc + elem_to_f32(arow[i]) * elem_to_f32(w[(int64_t)c * ldw + i]);     // the products are exact in fp32
        f32_to_elem(acc, orow[c]);
    }
}
template <class T, int K> static inline void ss_in_host(const AumStreamInArgs& a) {
    constexpr int NCH = (K + 511) / 512;
    std::vector<T> normed(K);
    for (int64_t r = 0; r < a.total; ++r) {
        const AumNormArgs p = ss_norm_args<T>(a, r, normed.data(), K, true);
        rmsnorm_fwd_vec<T, float, NCH>(p, 0);
        ss_dot_row<T>(normed.data(), static_cast<const T*>(a.w_in), a.ldw, 2 * a.dim, K, static_cast<T*>(a.xz) + r * a.xz_ts);
    }
}
template <class T, int K> static inline void ss_out_host(const AumStreamOutArgs& a) {
    for (int64_t r = 0; r < a.total; ++r)
        ss_dot_row<T>(static_cast<const T*>(a.y) + r * a.y_ts, static_cast<const T*>(a.w_out), a.ldw, a.d_model, K, static_cast<T*>(a.out) + r * a.out_ts);
}
#else
// ---- gfx950 ------------------------------------------------------------------------------------------------------------------------------
// the weight fragments of this wave and the products of one token tile
template <bool BF16, int K, int NF> struct SsMma {
    static constexpr int STEPS = K / 32, MAXS = (STEPS + SS_NW - 1) / SS_NW;
    static_assert(K % 32 == 0, "whole K-steps");
    aumx::s8v wf[NF][MAXS];
    int wv, lane, rho, kg;

    AUM_DEV void init(const void* w, int64_t ldw, int col0) {
        lane = (int)(threadIdx.x & 63u); wv = wave_in_wg(); rho = lane & 15; kg = lane >> 4;
        const aumx::s8v zero = {0, 0, 0, 0, 0, 0, 0, 0};
        const char* wb = static_cast<const char*>(w);
        AUM_UNROLL
        for (int f = 0; f < NF; ++f)
            AUM_UNROLL
            for (int i = 0; i < MAXS; ++i) {
                const int s = wv + SS_NW * i;
                wf[f][i] = s < STEPS ? *reinterpret_cast<const aumx::s8v*>(wb + ((int64_t)(col0 + f * 16 + rho) * ldw + s * 32 + kg * 8) * 2) : zero;
            }
    }
    // this lane's piece of the B operand of step wv + SS_NW i: 16 bytes at `row` + (32 step + 8 kg) elements; ok: the token row exists
    AUM_DEV void load_b(const char* row, bool ok, aumx::s8v (&bf)[MAXS]) const {
        const aumx::s8v zero = {0, 0, 0, 0, 0, 0, 0, 0};
        AUM_UNROLL
        for (int i = 0; i < MAXS; ++i) {
            const int s = wv + SS_NW * i;
            bf[i] = ok && s < STEPS ? *reinterpret_cast<const aumx::s8v*>(row + (s * 32 + kg * 8) * 2) : zero;
        }
    }
    // red: SS_NW * NF * 64 accumulators in LDS.  Every wave of the workgroup calls this the same number of times (two barriers inside).
    AUM_DEV void tile(const aumx::s8v (&bf)[MAXS], aumx::f4v* red, void* out, int64_t out_ts, int col0, int64_t t0, int total) const {
        aumx::f4v acc[NF];
        AUM_UNROLL
        for (int f = 0; f < NF; ++f) acc[f] = aumx::f4v{0.f, 0.f, 0.f, 0.f};
        AUM_UNROLL
        for (int i = 0; i < MAXS; ++i)
            if (wv + SS_NW * i < STEPS) {
                AUM_UNROLL
                for (int f = 0; f < NF; ++f) acc[f] = aumx::mfma<BF16>(wf[f][i], bf[i], acc[f]);
            }
        AUM_UNROLL
        for (int f = 0; f < NF; ++f) red[(wv * NF + f) * 64 + lane] = acc[f];
        __syncthreads();
        if (wv < NF) {
            aumx::f4v s = red[wv * 64 + lane];                                   // wave 0's partial of fragment wv
            AUM_UNROLL
            for (int w = 1; w < SS_NW; ++w) s = s + red[(w * NF + wv) * 64 + lane];
            if (t0 + rho < total) {
                aumx::u2v v;
                v.x = aumx::pack2<BF16>(s[0], s[1]);
                v.y = aumx::pack2<BF16>(s[2], s[3]);
                *reinterpret_cast<aumx::u2v*>(static_cast<char*>(out) + ((t0 + rho) * out_ts + col0 + wv * 16 + kg * 4) * 2) = v;
            }
        }
        __syncthreads();                                                         // red and the caller's tile are free again
    }
};

template <class T, bool BF16, int K>
__global__ __launch_bounds__(SS_NW * 64) void k_stream_in(AumStreamInArgs a) {
    constexpr int NF = SS_IN_NF, NCH = (K + 511) / 512, PITCH = K * 2 + 16;     // bytes per tile row: + 16 spreads the rows over the banks
    typedef SsMma<BF16, K, NF> M;
    __shared__ __attribute__((aligned(16))) char tile[SS_TILE * PITCH];
    __shared__ aumx::f4v red[SS_NW * NF * 64];
    const int col0 = (int)blockIdx.x * 16 * NF;
    M m;
    m.init(a.w_in, a.ldw, col0);
    for (int64_t t0 = 0; t0 < a.total; t0 += SS_TILE) {
        const AumNormArgs p = ss_norm_args<T>(a, t0, tile, PITCH / 2, blockIdx.x == 0);
        for (int r = m.wv; r < SS_TILE && t0 + r < a.total; r += SS_NW) rmsnorm_fwd_vec<T, float, NCH>(p, r);
        __syncthreads();
        aumx::s8v bf[M::MAXS];
        m.load_b(tile + m.rho * PITCH, t0 + m.rho < a.total, bf);
        m.tile(bf, red, a.xz, a.xz_ts, col0, t0, a.total);
    }
}

template <class T, bool BF16, int K>
__global__ __launch_bounds__(SS_NW * 64) void k_stream_out(AumStreamOutArgs a) {
    constexpr int NF = SS_OUT_NF;
    typedef SsMma<BF16, K, NF> M;
    __shared__ aumx::f4v red[SS_NW * NF * 64];
    const int col0 = (int)blockIdx.x * 16 * NF;
    M m;
    m.init(a.w_out, a.ldw, col0);
    for (int64_t t0 = 0; t0 < a.total; t0 += SS_TILE) {
        const bool ok = t0 + m.rho < a.total;
        aumx::s8v bf[M::MAXS];
        m.load_b(static_cast<const char*>(a.y) + (ok ? (t0 + m.rho) * a.y_ts * 2 : 0), ok, bf);
        m.tile(bf, red, a.out, a.out_ts, col0, t0, a.total);
    }
}
#endif

// one launch each; the operands have passed ss_in_check / ss_out_check
template <class T, bool BF16> static int ss_in_launch(const AumStreamInArgs& a, aum_stream_t s) {
    return with_int<192, 384, 768>(a.d_model, [&](auto k) {
        return AUM_LAUNCH(2 * a.dim / (16 * SS_IN_NF), SS_NW * 64, s, (NoLds{}), (k_stream_in<T, BF16, k>), (AUM_HOST_LOOP(ss_in_host<T, k>(a))), a);
    });
}
template <class T, bool BF16> static int ss_out_launch(const AumStreamOutArgs& a, aum_stream_t s) {
    return with_int<384, 768, 1536>(a.dim, [&](auto k) {
        return AUM_LAUNCH(a.d_model / (16 * SS_OUT_NF), SS_NW * 64, s, (NoLds{}), (k_stream_out<T, BF16, k>), (AUM_HOST_LOOP(ss_out_host<T, k>(a))), a);
    });
}
static inline int ss_in_run(const AumStreamInArgs& a, aum_stream_t s) {
    return a.dtype == AUM_BF16 ? ss_in_launch<bf16_t, true>(a, s) : ss_in_launch<f16_t, false>(a, s);
}
static inline int ss_out_run(const AumStreamOutArgs& a, aum_stream_t s) {
    return a.dtype == AUM_BF16 ? ss_out_launch<bf16_t, true>(a, s) : ss_out_launch<f16_t, false>(a, s);
}

// ---- the workspace of aum_stream_layers: byte offsets, each a multiple of 16 -----------------------------------------------------------
struct SsWs { int64_t xz, y, hid[2], res[2], block, block_bytes, total; };
static inline SsWs ss_ws(int64_t total, int d_model, int dim, int64_t block_bytes) {
    auto up = [](int64_t n) { return (n + 15) / 16 * 16; };
    SsWs w;
    w.xz = 0;
    w.y = w.xz + up(total * 2 * dim * 2);
    w.hid[0] = w.y + up(total * dim * 2);
    w.hid[1] = w.hid[0] + up(total * d_model * 2);
    w.res[0] = w.hid[1] + up(total * d_model * 2);
    w.res[1] = w.res[0] + up(total * d_model * 4);
    w.block = w.res[1] + up(total * d_model * 4);
    w.block_bytes = block_bytes;
    w.total = w.block + up(block_bytes);
    return w;
}

}  // namespace aum
