// stream_tm_kernels.h -- chunked streaming inference of the causal block: the conv window and the SSM state advanced by T >= 1 tokens per
// launch FROM CARRIED STATE (include/aum_hip.h: aum_conv1d_tm_chunk, aum_scan_tm_chunk).  Token-major activations (batch, T, dim), the
// caches fp32, contiguous and updated in place in the layouts Mamba.allocate_inference_cache returns: conv_state (batch, dim, width),
// state (batch, dim, dstate).  Results = T successive calls of the per-token kernels of decode_kernels.h.
//
// These are latency kernels (B = 1..8, E = 1536: 24..192 waves on 1024 SIMDs): one launch and one serial chain of T steps per wave, no LDS,
// no workgroup barriers, no atomics, waits left to the compiler.
//   * conv: the division of conv_tm_kernels.h -- a lane owns 16 bytes of consecutive channels, the window is four register rows -- seeded
//     from conv_state instead of from zero and written back to it behind the last step.
//   * scan: the division of scan_tm_kernels.h -- a wavefront owns 64 channels of one batch entry (lane = channel), the 16 states of a
//     channel live in registers for the whole call.  B_t / C_t are wave-uniform: lane n (mod 16) fetches element n of the step's rows and a
//     step takes its 32 values out of the two registers with v_readlane_b32, so they enter the arithmetic as scalar operands.
//   * two blocks of 8 steps of operands are in flight (requests past the chunk are clamped to its last row: no conditions around loads).
//
// PARTITION PROPERTY: advancing by T1 + T2 tokens in one call and by T1, then T2 gives bit-identical outputs and caches.  The carried
// state crosses calls as exact fp32 (the conv window holds the inputs themselves), and every step is the same instruction sequence on
// the same values wherever it falls in a call or in a block: one `step` body, no first / last step special cases, no re-association that
// depends on the block phase (the library is built with -ffp-contract=off).
//
// PACKED SESSIONS (aum_conv1d_tm_chunk_var, aum_scan_tm_chunk_var): the rows of several sessions behind one another in one (total, dim)
// stream, cu_seqlens saying where each session's rows are and state_indices which row of a pool of caches it owns.  The partition
// property extends to packing: a session's outputs and cache row are bit for bit what the fixed-batch kernel gives at batch 1 on those rows,
// whichever other sessions share the call, wherever it sits in the pack, whichever cache row it owns.  That holds by construction: ONE
// per-unit routine per operator (convc_unit, scanc_unit: a sequence's base pointers, its length, its cache row) holds the step; the
// fixed-batch kernel and the packed kernel differ only in where those arguments come from (b * X_bs / b-th cache row; cu_seqlens[i] * X_ts
// / cache row state_indices[i], wave-uniform values read with plain loads).  An empty sequence, an index outside the pool or a
// cu_seqlens pair outside [0, total] returns before anything is fetched.
//
// PEEK ROW (template parameter PEEK of the two units; AUM_CONV_PEEK_LAST / AUM_SCAN_PEEK_LAST / AUM_STREAM_PEEK_LAST): the last of a
// sequence's L rows is computed and stored like any other, and the cache is written as after L - 1 rows.  The block loop runs over the
// first L - 1 rows, the exit stores follow it (none for L == 1: the cache row is not touched), and then ONE more call of the same `step`
// takes the last row, fetched ahead of the loop, from the registers the exit stores have just read.  The window cannot be rebuilt
// behind the last step (it holds four inputs; the oldest is gone), so the early state is taken where it exists.  The cache crosses the
// exit as exact fp32, so the result is bit for bit a call on rows 0 .. L - 2 followed by an uncommitted call on row L - 1.  PEEK is a
// template parameter because scanc_unit fills the scalar file: with PEEK == false every added expression folds away and the existing
// kernels compile to what they were; the PEEK kernels are instantiations of their own.
//
// PEEK ROWS EVERY P ROWS (template parameter PEEKS of the two units with the period `pe` = P >= 1; aum_conv1d_tm_chunk_peeks /
// aum_scan_tm_chunk_peeks): row j of a sequence (counted from its first row in the call) is a peek row iff (j + 1) % (P + 1) == 0 -- a
// cls row behind every time column of a clip, all columns in one pass.  All L rows go through the block loop and the SAME `step`; a peek
// row's step leaves the carried registers alone: the conv does not move the window, the scan steps into temporaries (the vfma2 results
// the output is summed from) and does not copy them back.  Which rows those are depends on the row index only (a wave-uniform scalar:
// the index of the next peek row, moved on by P + 1 behind each), so a row is the same instruction sequence on the same fp32 values
// whether it commits or not, and per sequence y and the cache row are bit for bit the chain of PEEK (PEEK_LAST) calls on one group of
// P + 1 rows after the other, then a plain call on the trailing partial group.  The exit stores stay behind the loop and the fetch
// scheme is unchanged.  With PEEKS == false the added expressions fold away (as for PEEK); PEEK and PEEKS are never set together.
#pragma once
#include "conv_tm_kernels.h"
#include "scan_tm_kernels.h"

namespace aum {

constexpr int STREAM_UB = 8;       // steps fetched together; two such blocks in flight

// ---- conv ---------------------------------------------------------------------------------------
// what the units of one launch share
struct ConvcOps {
    const float *weight, *bias;
    int64_t x_ts, y_ts;
    int dim, width;
};

// unit = (sequence, block of 64 * V channels): L >= 1 rows at x / y (row stride x_ts / y_ts elements), the sequence's cache row `win`.
// commit == false (aum_stream_block_tm with AUM_STREAM_NO_COMMIT): the cache row is read and not written -- the exit stores are skipped
// PEEK: row L - 1 is a peek row -- LC = L - 1 rows go through the loop and into the cache, the last one is stepped behind the exit stores
// PEEKS: every (pe + 1)-th row is a peek row -- all L rows go through the loop, a peek row's step does not move the window
template <class T, bool SILU, bool PEEK = false, bool PEEKS = false>
AUM_DEV void convc_unit(const ConvcOps& a, const T* x, const T* y, float* win, int L, int cb, bool commit = true, int pe = 0) {
    static_assert(!(PEEK && PEEKS), "one peek row behind the rows, or one every pe rows");
    constexpr int V = convt_vec<T, false>(), NP = V / 2, ES = (int)sizeof(T), W = CONVT_W;
    AumConvTmArgs s = {};
    s.weight = a.weight;
    s.bias = a.bias;
    s.dim = a.dim;
    s.width = a.width;
    ConvtLane<T, false> ln;
    convt_lane_setup<T, false>(s, cb, ln);
    const gbuf<T> xb = make_gbuf(x);
    const gbuf<T> yb = make_gbuf(y);
    const int LC = PEEK ? L - 1 : L;             // the rows the cache takes in
    const vi coff = ln.c0 * ES;
    const int x_tb = (int)a.x_ts * ES, y_tb = (int)a.y_ts * ES;
    vf2 w2[W][NP], bias2[NP];
    AUM_UNROLL
    for (int p = 0; p < NP; ++p) {
        bias2[p] = mk2(ln.bias[2 * p], ln.bias[2 * p + 1]);
        AUM_UNROLL
        for (int k = 0; k < W; ++k) w2[k][p] = mk2(ln.w[k][2 * p], ln.w[k][2 * p + 1]);
    }
    // xr[i]: the input of step t - 4 + i before step t.  Entry: conv_state[j] is input j - width, so row i is conv_state[width - 4 + i]
    // (rows older than the cache are zero: they meet zero taps and are never written back).
    vf2 xr[W][NP];
    AUM_UNROLL
    for (int i = 0; i < W; ++i) {
        const int j = a.width - W + i;
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) {
            if (j >= 0) xr[i][p] = mk2(gload_u(win, (ln.c0 + 2 * p) * a.width + j), gload_u(win, (ln.c0 + 2 * p + 1) * a.width + j));
            else xr[i][p] = spl2(splat(0.f));
        }
    }
    auto unpack2 = [&](const convt_raw<T, false>& q, vf2 (&o)[NP]) {
        vf t[V];
        convt_unpack<T, false>(q, t);
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) o[p] = mk2(t[2 * p], t[2 * p + 1]);
    };
    const bool all_live = a.dim % (WAVE * V) == 0;
    auto load_blk = [&](int itb, convt_raw<T, false> (&raw)[STREAM_UB]) {
        AUM_UNROLL
        for (int j = 0; j < STREAM_UB; ++j) {
            const int it = itb + j < L ? itb + j : L - 1;
            raw[j] = convt_load<T, false>(xb, coff, it * x_tb);
        }
    };
    // one step: y = act(bias + w0 x[t-3] + w1 x[t-2] + w2 x[t-1] + w3 x[t]) in that order, then the window moves by one row (adv; a
    // peek row of PEEKS leaves it where it is)
    auto step = [&](int it, const convt_raw<T, false>& raw, bool adv) {
        vf2 xn[NP];
        unpack2(raw, xn);
        vf y[V];
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) {
            vf2 acc = bias2[p];
            AUM_UNROLL
            for (int k = 0; k < W - 1; ++k) acc = vfma2(w2[k][p], xr[k + 1][p], acc);
            acc = vfma2(w2[W - 1][p], xn[p], acc);
            if (SILU) acc = acc * vsigmoid2(acc);
            y[2 * p] = lo2(acc);
            y[2 * p + 1] = hi2(acc);
            if (!PEEKS || adv) {
                AUM_UNROLL
                for (int k = 0; k < W - 1; ++k) xr[k][p] = xr[k + 1][p];
                xr[W - 1][p] = xn[p];
            }
        }
        if (all_live) convt_store<T, false>(yb, coff, it * y_tb, y);
        else convt_store_m<T, false>(yb, coff, it * y_tb, y, ln.live);
    };
    int next_peek = pe;                         // PEEKS: the index of the next peek row
    auto comp_blk = [&](int itb, const convt_raw<T, false> (&raw)[STREAM_UB]) {
        AUM_UNROLL
        for (int j = 0; j < STREAM_UB; ++j) {
            if (itb + j < LC) {
                const bool pk = PEEKS && itb + j == next_peek;
                if (pk) next_peek += pe + 1;
                step(itb + j, raw[j], !pk);
            }
        }
    };
    convt_raw<T, false> ra[STREAM_UB], rb[STREAM_UB], rp;
    if (PEEK) rp = convt_load<T, false>(xb, coff, (L - 1) * x_tb);
    load_blk(0, ra);            // requests are clamped to row L - 1, which exists: an empty loop (PEEK, L == 1) fetches that row only
    for (int itb = 0; itb < LC; itb += 2 * STREAM_UB) {
        load_blk(itb + STREAM_UB, rb);
        comp_blk(itb, ra);
        load_blk(itb + 2 * STREAM_UB, ra);
        comp_blk(itb + STREAM_UB, rb);
    }
    // exit: conv_state[j] = input LC - width + j = row 4 - width + j
    if (commit && (!PEEK || LC > 0)) {
        AUM_UNROLL
        for (int i = 0; i < W; ++i) {
            const int j = a.width - W + i;
            if (j >= 0) {
                AUM_UNROLL
                for (int p = 0; p < NP; ++p) {
                    gstore(win, (ln.c0 + 2 * p) * a.width + j, lo2(xr[i][p]), ln.live);
                    gstore(win, (ln.c0 + 2 * p + 1) * a.width + j, hi2(xr[i][p]), ln.live);
                }
            }
        }
    }
    if (PEEK) step(L - 1, rp, true);
}

// fixed batch: unit = (batch entry, channel block), channel block fastest
template <class T, bool SILU>
AUM_DEV void convc_wave(const AumConvTmChunkArgs& a, int wg) {
    const int ncb = convt_cblocks<T, false>(a.dim);
    const int cb = wg % ncb, b = wg / ncb;
    const ConvcOps o = {a.weight, a.bias, a.x_ts, a.y_ts, a.dim, a.width};
    convc_unit<T, SILU>(o, row_ptr<T>(a.x, (int64_t)b * a.x_bs), row_ptr<T>(a.y, (int64_t)b * a.y_bs), a.conv_state + (int64_t)b * a.dim * a.width,
                        a.len, cb);
}

// rows [r0, r1) and the cache row of sequence i of a packed call; false: the sequence is a no-op (empty, a cache row outside the pool, or
// a cu_seqlens pair that is not inside [0, total]) and nothing of it may be touched
AUM_DEV bool stream_seq(const int32_t* cu_seqlens, const int32_t* state_indices, int i, int total, int nrows, int& r0, int& len, int& row) {
    r0 = cu_seqlens[i];
    const int r1 = cu_seqlens[i + 1];
    row = state_indices ? state_indices[i] : i;
    len = r1 - r0;
    return r0 >= 0 && r1 <= total && len > 0 && row >= 0 && row < nrows;
}

// packed sessions: unit = (sequence, channel block), channel block fastest
template <class T, bool SILU, bool PEEK = false, bool PEEKS = false>
AUM_DEV void convc_var_wave(const AumConvTmChunkVarArgs& a, int wg, int pe = 0) {
    const int ncb = convt_cblocks<T, false>(a.dim);
    const int cb = wg % ncb, i = wg / ncb;
    int r0, len, row;
    if (!stream_seq(a.cu_seqlens, a.state_indices, i, a.total, a.nrows, r0, len, row)) return;
    const ConvcOps o = {a.weight, a.bias, a.x_ts, a.y_ts, a.dim, a.width};
    convc_unit<T, SILU, PEEK, PEEKS>(o, row_ptr<T>(a.x, (int64_t)r0 * a.x_ts), row_ptr<T>(a.y, (int64_t)r0 * a.y_ts),
                                     a.conv_state + (int64_t)row * a.dim * a.width, len, cb, true, pe);
}

// ---- scan ---------------------------------------------------------------------------------------
struct ScancRaw { vi u, d, z, b, c; };      // one step's operands as loaded (widened where they are used)

// what the units of one launch share (row strides in elements)
struct ScancOps {
    const float *A, *D, *delta_bias;
    int64_t u_ts, delta_ts, z_ts, B_ts, C_ts, out_ts;
};
// one sequence: its first row in every operand, its cache row, its length
template <class T> struct ScancSeq {
    const T *u, *delta, *z, *B, *C, *out;
    const float* state;
    int len;
};

// unit = (sequence, group of 64 channels from e0).  SP: delta = softplus(delta + bias); otherwise delta + bias (an activated delta comes
// with bias == NULL: the launcher drops it).  commit == false: the state row is read and not written (the exit stores are skipped).
// PEEK: row L - 1 is a peek row -- LC = L - 1 rows go through the loop and into the state, the last one is stepped behind the exit stores
// PEEKS: every (pe + 1)-th row is a peek row -- all L rows go through the loop, a peek row's step does not take its result into the state
// CKPT (aum_scan_tm_peeks_fwd_ckpt, the training forward; with PEEKS): the sequence enters with a ZERO state (q.state is not read), and the
// fp32 state in front of rows 0, 8, 16, ... is stored to ck + (row / 8) * ck_sb bytes in the (dim, 16) layout of a cache row; commit is false
template <class T, bool SP, bool HAS_Z, bool PEEK = false, bool PEEKS = false, bool CKPT = false>
AUM_DEV void scanc_unit(const ScancOps& p, const ScancSeq<T>& q, int e0, bool commit = true, int pe = 0, const float* ck = nullptr, int ck_sb = 0) {
    static_assert(!(PEEK && PEEKS), "one peek row behind the rows, or one every pe rows");
    static_assert(!CKPT || PEEKS, "the checkpointing form is the training forward of the PEEKS rows");
    constexpr int N = SCANT_N, ES = (int)sizeof(T);
    const int L = q.len;
    const int LC = PEEK ? L - 1 : L;             // the rows the state takes in
    const vi lane = lane_id();
    const vi ec = lane + e0;                     // dim % 64 == 0: every lane is a channel
    vf2 A2[N / 2];                               // A * log2(e), states (2j, 2j+1)
    AUM_UNROLL
    for (int j = 0; j < N / 2; ++j) A2[j] = mk2(gload_u(p.A, ec * N + 2 * j) * LOG2E, gload_u(p.A, ec * N + 2 * j + 1) * LOG2E);
    const vf biasv = p.delta_bias ? gload_u(p.delta_bias, ec) : splat(0.f);
    const vf Dv = p.D ? gload_u(p.D, ec) : splat(0.f);
    const gbuf<T> ubuf = make_gbuf(q.u);
    const gbuf<T> dbuf = make_gbuf(q.delta);
    const gbuf<T> zbuf = make_gbuf(HAS_Z ? q.z : q.u);
    const gbuf<T> obuf = make_gbuf(q.out);
    const gbuf<T> Bbuf = make_gbuf(q.B);
    const gbuf<T> Cbuf = make_gbuf(q.C);
    const gbuf<float> sbuf = make_gbuf(CKPT ? ck : q.state);
    const int u_tb = (int)p.u_ts * ES, d_tb = (int)p.delta_ts * ES, z_tb = HAS_Z ? (int)p.z_ts * ES : 0, o_tb = (int)p.out_ts * ES,
              B_tb = (int)p.B_ts * ES, C_tb = (int)p.C_ts * ES;
    const vi el_off = ec * ES;                   // this lane's channel inside a token row
    const vi bc_off = (lane & (N - 1)) * ES;     // the element of a B / C row this lane fetches
    const vi st_off = ec * (N * 4);              // this lane's 16 states: 64 contiguous bytes
    // entry state
    vf2 x[N / 2];
    AUM_UNROLL
    for (int i = 0; i < N / 4; ++i) {
        vf t[4];
        if (CKPT) t[0] = t[1] = t[2] = t[3] = splat(0.f);
        else vq_unpack<float>(gbuf_load16(sbuf, st_off + 16 * i, 0), t);
        x[2 * i] = mk2(t[0], t[1]);
        x[2 * i + 1] = mk2(t[2], t[3]);
    }
    auto load_blk = [&](int itb, ScancRaw (&raw)[STREAM_UB]) {
        AUM_UNROLL
        for (int j = 0; j < STREAM_UB; ++j) {
            const int it = itb + j < L ? itb + j : L - 1;
            raw[j].u = gbuf_load_raw(ubuf, el_off, it * u_tb);
            raw[j].d = gbuf_load_raw(dbuf, el_off, it * d_tb);
            if (HAS_Z) raw[j].z = gbuf_load_raw(zbuf, el_off, it * z_tb);
            raw[j].b = gbuf_load_raw(Bbuf, bc_off, it * B_tb);
            raw[j].c = gbuf_load_raw(Cbuf, bc_off, it * C_tb);
        }
    };
    // one step (the arithmetic of scant_fwd_run's `step`, stage by stage over the eight state pairs):
    //   dl = softplus?(delta + bias);  a = exp2(dl A log2e);  x = a x + (dl u) B;  y = <x, C> + D u;  out = y z sigmoid(z)
    // The new state is formed in xn and the output summed from it; adv: it becomes the state (a peek row of PEEKS drops it)
    auto step = [&](int it, const ScancRaw& r, bool adv) {
        vf dl = raw_to_f32<T>(r.d) + biasv;
        if (SP) dl = vsoftplus(dl);
        const vf uu = raw_to_f32<T>(r.u);
        const vf du = dl * uu;
        const vf bv = raw_to_f32<T>(r.b), cv = raw_to_f32<T>(r.c);
        const vf2 dl2 = spl2(dl), du2 = spl2(du);
        vf2 a[N / 2], Bp[N / 2], Cp[N / 2], xn[N / 2];
        AUM_UNROLL
        for (int j = 0; j < N / 2; ++j) {
            Bp[j] = mk2(splat(readlane(bv, 2 * j)), splat(readlane(bv, 2 * j + 1)));
            Cp[j] = mk2(splat(readlane(cv, 2 * j)), splat(readlane(cv, 2 * j + 1)));
        }
        AUM_UNROLL
        for (int j = 0; j < N / 2; ++j) a[j] = dl2 * A2[j];
        vf zz = splat(0.f), ez = splat(0.f);
        if (HAS_Z) {
            zz = raw_to_f32<T>(r.z);
            ez = zz * (-LOG2E);
        }
        AUM_UNROLL
        for (int j = 0; j < N / 2; ++j) Bp[j] = du2 * Bp[j];
        AUM_UNROLL
        for (int j = 0; j < N / 2; ++j) a[j] = vexp2_2(a[j]);
        if (HAS_Z) ez = vexp2(ez);
        AUM_UNROLL
        for (int j = 0; j < N / 2; ++j) xn[j] = vfma2(a[j], x[j], Bp[j]);
        vf sg = splat(1.f);
        if (HAS_Z) sg = vrcp(ez + 1.0f);
        vf2 y2[4];
        AUM_UNROLL
        for (int j = 0; j < 4; ++j) y2[j] = xn[j] * Cp[j];
        AUM_UNROLL
        for (int j = 4; j < N / 2; ++j) y2[j & 3] = vfma2(xn[j], Cp[j], y2[j & 3]);
        if (!PEEKS || adv) {
            AUM_UNROLL
            for (int j = 0; j < N / 2; ++j) x[j] = xn[j];
        }
        const vf2 ysum = (y2[0] + y2[1]) + (y2[2] + y2[3]);
        const vf ys = lo2(ysum) + hi2(ysum);
        vf tot = vfma(uu, Dv, ys);
        if (HAS_Z) tot = tot * (zz * sg);
        gbuf_store(obuf, el_off, it * o_tb, tot);
    };
    int next_peek = pe;                         // PEEKS: the index of the next peek row
    auto comp_blk = [&](int itb, const ScancRaw (&raw)[STREAM_UB]) {
        if (CKPT && itb < LC) {                 // the state in front of the block (itb is a multiple of STREAM_UB)
            AUM_UNROLL
            for (int i = 0; i < N / 4; ++i) {
                const vf t[4] = {lo2(x[2 * i]), hi2(x[2 * i]), lo2(x[2 * i + 1]), hi2(x[2 * i + 1])};
                gbuf_store16(sbuf, st_off + 16 * i, (itb / STREAM_UB) * ck_sb, vq_pack<float>(t));
            }
        }
        AUM_UNROLL
        for (int j = 0; j < STREAM_UB; ++j) {
            if (itb + j < LC) {
                const bool pk = PEEKS && itb + j == next_peek;
                if (pk) next_peek += pe + 1;
                step(itb + j, raw[j], !pk);
            }
        }
    };
    ScancRaw ra[STREAM_UB], rb[STREAM_UB];
    load_blk(0, ra);            // requests are clamped to row L - 1, which exists: an empty loop (PEEK, L == 1) fetches that row only
    for (int itb = 0; itb < LC; itb += 2 * STREAM_UB) {
        load_blk(itb + STREAM_UB, rb);
        comp_blk(itb, ra);
        load_blk(itb + 2 * STREAM_UB, ra);
        comp_blk(itb + STREAM_UB, rb);
    }
    ScancRaw rp;                // the peek row, fetched here and not ahead of the loop: five more live registers across it are not free in this kernel
    if (PEEK) {
        const int it = L - 1;
        rp.u = gbuf_load_raw(ubuf, el_off, it * u_tb);
        rp.d = gbuf_load_raw(dbuf, el_off, it * d_tb);
        if (HAS_Z) rp.z = gbuf_load_raw(zbuf, el_off, it * z_tb);
        rp.b = gbuf_load_raw(Bbuf, bc_off, it * B_tb);
        rp.c = gbuf_load_raw(Cbuf, bc_off, it * C_tb);
    }
    // exit state
    if (commit && (!PEEK || LC > 0)) {
        AUM_UNROLL
        for (int i = 0; i < N / 4; ++i) {
            const vf t[4] = {lo2(x[2 * i]), hi2(x[2 * i]), lo2(x[2 * i + 1]), hi2(x[2 * i + 1])};
            gbuf_store16(sbuf, st_off + 16 * i, 0, vq_pack<float>(t));
        }
    }
    if (PEEK) step(L - 1, rp, true);
}

// fixed batch: unit = (batch entry, group of 64 channels), channel group fastest
template <class T, bool SP, bool HAS_Z>
AUM_DEV void scanc_wave(const AumScanTmChunkArgs& p, int wg) {
    const int ngrp = p.dim / WAVE;
    const int e0 = (wg % ngrp) * WAVE, b = wg / ngrp;
    const ScancOps o = {p.A, p.D, p.delta_bias, p.u_ts, p.delta_ts, p.z_ts, p.B_ts, p.C_ts, p.out_ts};
    const ScancSeq<T> q = {row_ptr<T>(p.u, (int64_t)b * p.u_bs), row_ptr<T>(p.delta, (int64_t)b * p.delta_bs),
                           HAS_Z ? row_ptr<T>(p.z, (int64_t)b * p.z_bs) : nullptr, row_ptr<T>(p.B, (int64_t)b * p.B_bs),
                           row_ptr<T>(p.C, (int64_t)b * p.C_bs), row_ptr<T>(p.out, (int64_t)b * p.out_bs),
                           p.state + (int64_t)b * p.dim * SCANT_N, p.len};
    scanc_unit<T, SP, HAS_Z>(o, q, e0);
}

// packed sessions: unit = (sequence, group of 64 channels), channel group fastest
template <class T, bool SP, bool HAS_Z, bool PEEK = false, bool PEEKS = false>
AUM_DEV void scanc_var_wave(const AumScanTmChunkVarArgs& p, int wg, int pe = 0) {
    const int ngrp = p.dim / WAVE;
    const int e0 = (wg % ngrp) * WAVE, i = wg / ngrp;
    int r0, len, row;
    if (!stream_seq(p.cu_seqlens, p.state_indices, i, p.total, p.nrows, r0, len, row)) return;
    const ScancOps o = {p.A, p.D, p.delta_bias, p.u_ts, p.delta_ts, p.z_ts, p.B_ts, p.C_ts, p.out_ts};
    const ScancSeq<T> q = {row_ptr<T>(p.u, (int64_t)r0 * p.u_ts), row_ptr<T>(p.delta, (int64_t)r0 * p.delta_ts),
                           HAS_Z ? row_ptr<T>(p.z, (int64_t)r0 * p.z_ts) : nullptr, row_ptr<T>(p.B, (int64_t)r0 * p.B_ts),
                           row_ptr<T>(p.C, (int64_t)r0 * p.C_ts), row_ptr<T>(p.out, (int64_t)r0 * p.out_ts),
                           p.state + (int64_t)row * p.dim * SCANT_N, len};
    scanc_unit<T, SP, HAS_Z, PEEK, PEEKS>(o, q, e0, true, pe);
}

}  // namespace aum
