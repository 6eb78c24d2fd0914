// stream_train_kernels.h -- TIMELINE TRAINING: the adjoints of the peek-row operators of stream_tm_kernels.h (include/aum_hip.h:
// aum_scan_tm_peeks_fwd_ckpt, aum_scan_tm_peeks_bwd, aum_conv1d_tm_peeks_bwd).  Packed sequences (cu_seqlens), every sequence from a ZERO
// conv window and a ZERO state; row j of a sequence is a peek row iff (j + 1) % (P + 1) == 0 and a committed row otherwise.  One launch
// each, one wave per unit, no LDS, no workgroup barriers, no atomics, waits left to the compiler: results are bitwise repeatable and a
// sequence's results do not depend on its neighbours or its place in the pack.
//
//   * forward with checkpoints: scanc_unit<PEEKS, CKPT> -- the step of the inference kernel, so `out` is bit for bit that of
//     aum_scan_tm_chunk_peeks on a zeroed pool; the fp32 state in front of every STREAM_UB = 8 rows goes to the checkpoint buffer.  Slot
//     of block k of sequence i: cu_seqlens[i] / 8 + i + k (distinct for all blocks of a pack: floor(a) + ceil(b) <= floor(a + b) + 1), a slot is
//     (dim, 16) fp32 in the layout of a cache row; total / 8 + nseq slots in all.
//   * scan backward: unit = (sequence, 64 channels), lane = channel.  Blocks of 8 rows from the last to the first.  Per block: the rows'
//     operands are fetched and decoded once; then a loop over the eight state PAIRS -- the pair's states are rebuilt from the block's
//     checkpoint (the same a = exp2(dl A log2e), hn = a h + (dl u) B as the forward, so hn is the forward's bit for bit), then the adjoint
//     sweeps the block downward; g (dL/dh behind the row) and dA of the pair live in register vectors indexed by the loop counter.  dB | dC
//     terms of a pair (8 rows x 2 states) are summed over the 64 channels by the transposing butterfly (wave_sum16) and stored as one fp32
//     partial row per (channel group, token): [group][total][dB 16 | dC 16]; dA / dD / ddelta_bias leave one partial row per (sequence,
//     channel group): [seq][dim][16], [seq][dim], [seq][dim].  The caller adds groups / sequences with aum_sum_rows.  Every running sum
//     (dA, dD, ddelta_bias, g) takes its rows in strictly descending order, and a row whose dout is zero adds exact zeros: with dout zero on
//     the peek rows the committed rows' gradients are those of the sequence without its peek rows, bit for bit.
//   * conv backward: unit = (sequence, block of 64 * V channels), the fetch scheme and the step order of convc_unit (rows ascending, two
//     blocks of 8 rows of x and dy in flight).  A row recomputes its pre-activation from the window registers (the forward's fma order),
//     dpre = dy act'(pre); dw / db accumulate; the dx ADJOINT of the three committed rows in the window lives in registers and a row's dx
//     is stored when the row leaves the window (behind the third committed row after it; a peek row never enters it and stores w[3] dpre
//     at once); the three rows left at the end are flushed.  Ascending rows carry the forward's window, which the recomputed
//     pre-activation needs in any case, so every row of x and dy is fetched once; a descending walk would fetch the three committed
//     predecessors of every row a second time.  The sums are the same and their order is fixed.  dw / db: one partial row per sequence,
//     [seq][dim][width] and [seq][dim].
#pragma once
#include "stream_tm_kernels.h"

namespace aum {

// checkpoint slots of a pack / the first slot of sequence i whose first row is r0
AUM_HOSTDEV int64_t scanp_ck_slots(int64_t total, int64_t nseq) { return total / STREAM_UB + nseq; }
AUM_HOSTDEV int64_t scanp_ck_slot0(int64_t r0, int64_t i) { return r0 / STREAM_UB + i; }

// rows [r0, r0 + len) of sequence i of a pack without a pool; false: a no-op
AUM_DEV bool train_seq(const int32_t* cu_seqlens, int i, int total, int& r0, int& len) {
    r0 = cu_seqlens[i];
    const int r1 = cu_seqlens[i + 1];
    len = r1 - r0;
    return r0 >= 0 && r1 <= total && len > 0;
}

// ---- scan forward with checkpoints: unit = (sequence, group of 64 channels), channel group fastest -------------------------------------
template <class T, bool SP, bool HAS_Z>
AUM_DEV void scanp_fwd_wave(const AumScanTmChunkVarArgs& p, float* ckpt, int wg, int pe) {
    const int ngrp = p.dim / WAVE;
    const int e0 = (wg % ngrp) * WAVE, i = wg / ngrp;
    int r0, len;
    if (!train_seq(p.cu_seqlens, i, p.total, r0, len)) return;
    const ScancOps o = {p.A, p.D, p.delta_bias, p.u_ts, p.delta_ts, p.z_ts, p.B_ts, p.C_ts, p.out_ts};
    const ScancSeq<T> q = {row_ptr<T>(p.u, (int64_t)r0 * p.u_ts), row_ptr<T>(p.delta, (int64_t)r0 * p.delta_ts),
                           HAS_Z ? row_ptr<T>(p.z, (int64_t)r0 * p.z_ts) : nullptr, row_ptr<T>(p.B, (int64_t)r0 * p.B_ts),
                           row_ptr<T>(p.C, (int64_t)r0 * p.C_ts), row_ptr<T>(p.out, (int64_t)r0 * p.out_ts), nullptr, len};
    const int ck_sb = p.dim * SCANT_N * 4;
    scanc_unit<T, SP, HAS_Z, false, true, true>(o, q, e0, false, pe, ckpt + scanp_ck_slot0(r0, i) * (int64_t)(p.dim * SCANT_N), ck_sb);
}

// ---- scan backward -----------------------------------------------------------------------------------------------------------------------
constexpr int SCANP_RAW = 0, SCANP_SOFTPLUS = 1, SCANP_ACTIVATED = 2;        // delta + bias | softplus(delta + bias) | delta is softplus(raw + bias)

struct ScanpBwdOuts {
    void *du, *ddelta, *dz;
    float *dbc_part, *dA_part, *dD_part, *dbias_part;
    int64_t du_ts, ddelta_ts, dz_ts;
};

// p.out is dout.  The gradients of the rows are in the activation dtype; ddelta is in raw space (times the softplus derivative
// 1 - exp(-dl) for SCANP_SOFTPLUS / SCANP_ACTIVATED).
template <class T, int SPM, bool HAS_Z>
AUM_DEV void scanp_bwd_wave(const AumScanTmChunkVarArgs& p, const float* ckpt, const ScanpBwdOuts& w, int wg, int pe) {
    constexpr int N = SCANT_N, ES = (int)sizeof(T), UB = STREAM_UB;
    const int ngrp = p.dim / WAVE;
    const int grp = wg % ngrp, e0 = grp * WAVE, i = wg / ngrp;
    int r0, L;
    if (!train_seq(p.cu_seqlens, i, p.total, r0, L)) return;
    const vi lane = lane_id();
    const vi ec = lane + e0;
    const vf biasv = (SPM != SCANP_ACTIVATED && p.delta_bias) ? gload_u(p.delta_bias, ec) : splat(0.f);
    const vf Dv = p.D ? gload_u(p.D, ec) : splat(0.f);
    const gbuf<T> ubuf = make_gbuf(row_ptr<T>(p.u, (int64_t)r0 * p.u_ts));
    const gbuf<T> dbuf = make_gbuf(row_ptr<T>(p.delta, (int64_t)r0 * p.delta_ts));
    const gbuf<T> zbuf = make_gbuf(HAS_Z ? row_ptr<T>(p.z, (int64_t)r0 * p.z_ts) : row_ptr<T>(p.u, (int64_t)r0 * p.u_ts));
    const gbuf<T> gobuf = make_gbuf(row_ptr<T>(p.out, (int64_t)r0 * p.out_ts));
    const gbuf<T> Bbuf = make_gbuf(row_ptr<T>(p.B, (int64_t)r0 * p.B_ts));
    const gbuf<T> Cbuf = make_gbuf(row_ptr<T>(p.C, (int64_t)r0 * p.C_ts));
    const gbuf<T> dubuf = make_gbuf(row_ptr<T>(w.du, (int64_t)r0 * w.du_ts));
    const gbuf<T> ddbuf = make_gbuf(row_ptr<T>(w.ddelta, (int64_t)r0 * w.ddelta_ts));
    const gbuf<T> dzbuf = make_gbuf(HAS_Z ? row_ptr<T>(w.dz, (int64_t)r0 * w.dz_ts) : row_ptr<T>(w.du, (int64_t)r0 * w.du_ts));
    const float* ck = ckpt + scanp_ck_slot0(r0, i) * (int64_t)(p.dim * N);
    float* dbc = w.dbc_part + ((int64_t)grp * p.total + r0) * (2 * N);
    const int u_tb = (int)p.u_ts * ES, d_tb = (int)p.delta_ts * ES, z_tb = HAS_Z ? (int)p.z_ts * ES : 0, go_tb = (int)p.out_ts * ES,
              B_tb = (int)p.B_ts * ES, C_tb = (int)p.C_ts * ES, du_tb = (int)w.du_ts * ES, dd_tb = (int)w.ddelta_ts * ES,
              dz_tb = HAS_Z ? (int)w.dz_ts * ES : 0;
    const vi el_off = ec * ES;
    const vi bc_off = (lane & (N - 1)) * ES;
    // the butterfly's result layout: lane l holds value k = (step k >> 1 of the block, state k & 1 of the pair); one lane of a quad stores
    const vi kq = ((lane >> 3) & 1) * 8 + ((lane >> 2) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 5) & 1);
    const vi ks = kq >> 1;
    const vi kslot = ks * (2 * N) + (kq & 1);
    const vm kfirst = (lane & 3) == 0;
    vf16 gg, dAacc;                              // dL/dh behind the current row and dA, the 16 states of the lane's channel
    AUM_UNROLL
    for (int n = 0; n < N; ++n) {
        vf16_set(gg, n, splat(0.f));
        vf16_set(dAacc, n, splat(0.f));
    }
    vf dDacc = splat(0.f), dbacc = splat(0.f);
    const int nblk = (L + UB - 1) / UB;
    for (int kb = nblk - 1; kb >= 0; --kb) {
        const int tb = kb * UB;
        const int nrow = L - tb < UB ? L - tb : UB;
        // ---- the block's rows: operands, dl, dl u, dy = dout z sigmoid(z), the factor of dz ----
        vf dl[UB], uu[UB], du[UB], dy[UB], dzf[UB], bv[UB], cv[UB], yacc[UB];
        vf2 S1[UB], S2[UB];                     // sum_n dhn B[n] and sum_n dhn A a h, the pair's halves added behind the passes
        bool cm[UB];                            // the row commits its state
        {
            int ph = (tb + 1) % (pe + 1);       // (row + 1) % (P + 1) of the block's first row
            vi ru[UB], rd[UB], rz[UB], rg[UB], rb[UB], rc[UB];
            AUM_UNROLL
            for (int s = 0; s < UB; ++s) {
                const int it = tb + s < L ? tb + s : L - 1;
                ru[s] = gbuf_load_raw(ubuf, el_off, it * u_tb);
                rd[s] = gbuf_load_raw(dbuf, el_off, it * d_tb);
                if (HAS_Z) rz[s] = gbuf_load_raw(zbuf, el_off, it * z_tb);
                rg[s] = gbuf_load_raw(gobuf, el_off, it * go_tb);
                rb[s] = gbuf_load_raw(Bbuf, bc_off, it * B_tb);
                rc[s] = gbuf_load_raw(Cbuf, bc_off, it * C_tb);
                cm[s] = ph != 0;
                ph = ph == pe ? 0 : ph + 1;
            }
            AUM_UNROLL
            for (int s = 0; s < UB; ++s) {
                vf d = raw_to_f32<T>(rd[s]) + biasv;
                if (SPM == SCANP_SOFTPLUS) d = vsoftplus(d);
                dl[s] = d;
                uu[s] = raw_to_f32<T>(ru[s]);
                du[s] = d * uu[s];
                bv[s] = raw_to_f32<T>(rb[s]);
                cv[s] = raw_to_f32<T>(rc[s]);
                const vf go = raw_to_f32<T>(rg[s]);
                if (HAS_Z) {
                    const vf zz = raw_to_f32<T>(rz[s]);
                    const vf sg = vsigmoid(zz);
                    dy[s] = go * (zz * sg);
                    dzf[s] = go * (sg * vfma(zz, splat(1.f) - sg, splat(1.f)));
                } else {
                    dy[s] = go;
                    dzf[s] = splat(0.f);
                }
                yacc[s] = splat(0.f);
                S1[s] = S2[s] = spl2(splat(0.f));
            }
        }
        // ---- passes over the state pairs (a real loop: the pairs' carries sit in register vectors indexed by the counter) ----
        _Pragma("nounroll")
        for (int j = 0; j < N / 2; ++j) {
            const vf2 Aj = mk2(gload_u(p.A, ec * N + 2 * j), gload_u(p.A, ec * N + 2 * j + 1));
            const vf2 A2j = Aj * spl2(splat(LOG2E));
            vf2 h = mk2(gload_u(ck, ec * N + 2 * j + kb * (p.dim * N)), gload_u(ck, ec * N + 2 * j + 1 + kb * (p.dim * N)));
            vf2 gj = mk2(vf16_get(gg, 2 * j), vf16_get(gg, 2 * j + 1)), dAj = mk2(vf16_get(dAacc, 2 * j), vf16_get(dAacc, 2 * j + 1));
            vf2 a[UB], wv[UB];                  // a = exp(dl A);  wv = a h, h the state in front of the row
            vf pc[2 * UB], pb[2 * UB];
            // forward sweep: the states of the block's rows as the forward formed them
            AUM_UNROLL
            for (int s = 0; s < UB; ++s) {
                pc[2 * s] = pc[2 * s + 1] = splat(0.f);
                pb[2 * s] = pb[2 * s + 1] = splat(0.f);
                if (s < nrow) {
                    const vf2 Bp = mk2(splat(readlane(bv[s], 2 * j)), splat(readlane(bv[s], 2 * j + 1)));
                    const vf2 Cp = mk2(splat(readlane(cv[s], 2 * j)), splat(readlane(cv[s], 2 * j + 1)));
                    a[s] = vexp2_2(spl2(dl[s]) * A2j);
                    wv[s] = a[s] * h;
                    const vf2 hn = vfma2(a[s], h, spl2(du[s]) * Bp);
                    const vf2 pcs = hn * spl2(dy[s]);          // dC[n] terms
                    pc[2 * s] = lo2(pcs);
                    pc[2 * s + 1] = hi2(pcs);
                    if (HAS_Z) {
                        const vf2 yc = hn * Cp;
                        yacc[s] = yacc[s] + (lo2(yc) + hi2(yc));
                    }
                    if (cm[s]) h = hn;
                }
            }
            const vf dCsum = wave_sum16(pc);
            // reverse sweep
            AUM_UNROLL
            for (int s = UB - 1; s >= 0; --s) {
                if (s < nrow) {
                    const vf2 Bp = mk2(splat(readlane(bv[s], 2 * j)), splat(readlane(bv[s], 2 * j + 1)));
                    const vf2 Cp = mk2(splat(readlane(cv[s], 2 * j)), splat(readlane(cv[s], 2 * j + 1)));
                    vf2 dhn = Cp * spl2(dy[s]);
                    if (cm[s]) dhn = dhn + gj;
                    const vf2 pbs = dhn * spl2(du[s]);         // dB[n] terms
                    pb[2 * s] = lo2(pbs);
                    pb[2 * s + 1] = hi2(pbs);
                    S1[s] = vfma2(dhn, Bp, S1[s]);
                    const vf2 r = dhn * wv[s];
                    S2[s] = vfma2(Aj, r, S2[s]);
                    dAj = vfma2(spl2(dl[s]), r, dAj);
                    if (cm[s]) gj = a[s] * dhn;
                    else gj = vfma2(a[s], dhn, gj);
                }
            }
            const vf dBsum = wave_sum16(pb);
            const vm st = kfirst && (ks < nrow);
            gstore(dbc, kslot + (tb * (2 * N) + 2 * j), dBsum, st);
            gstore(dbc, kslot + (tb * (2 * N) + 2 * j + N), dCsum, st);
            vf16_set(gg, 2 * j, lo2(gj));
            vf16_set(gg, 2 * j + 1, hi2(gj));
            vf16_set(dAacc, 2 * j, lo2(dAj));
            vf16_set(dAacc, 2 * j + 1, hi2(dAj));
        }
        // ---- the block's du, ddelta, dz; dD and ddelta_bias take the rows in descending order like every other running sum ----
        AUM_UNROLL
        for (int s = UB - 1; s >= 0; --s) {
            if (s < nrow) {
                const vf s1 = lo2(S1[s]) + hi2(S1[s]), s2 = lo2(S2[s]) + hi2(S2[s]);
                const vf duo = vfma(Dv, dy[s], dl[s] * s1);
                vf dd = vfma(uu[s], s1, s2);
                if (SPM != SCANP_RAW) dd = dd * vsigmoid_of_softplus(dl[s]);       // sigmoid(raw) = 1 - exp(-softplus(raw))
                dDacc = vfma(dy[s], uu[s], dDacc);
                dbacc = dbacc + dd;
                gbuf_store(dubuf, el_off, (tb + s) * du_tb, duo);
                gbuf_store(ddbuf, el_off, (tb + s) * dd_tb, dd);
                if (HAS_Z) gbuf_store(dzbuf, el_off, (tb + s) * dz_tb, dzf[s] * vfma(Dv, uu[s], yacc[s]));
            }
        }
    }
    const vm all = lane >= 0;
    float* dAp = w.dA_part + (int64_t)i * p.dim * N;
    AUM_UNROLL
    for (int n = 0; n < N; ++n) gstore(dAp, ec * N + n, vf16_get(dAacc, n), all);
    if (w.dD_part) gstore(w.dD_part + (int64_t)i * p.dim, ec, dDacc, all);
    if (w.dbias_part) gstore(w.dbias_part + (int64_t)i * p.dim, ec, dbacc, all);
}

// ---- conv backward: unit = (sequence, block of 64 * V channels), channel block fastest ----------------------------------------------------
struct ConvpBwdArgs {
    const void *x, *dy;
    const float *weight, *bias;
    void* dx;
    float *dw_part, *db_part;
    const int32_t* cu_seqlens;
    int64_t x_ts, dy_ts, dx_ts;
    int total, dim, width, pe;
};

// Registers: the fp32 instantiations hold four channels of 16-byte rows and sit at 245 (no SiLU) / 253 (SiLU) VGPRs of 256 with no scratch
// (16-bit: 151 - 173).  Anything added to the live set of the step (a third block in flight, a wider window) spills there: read hipcc's
// resource remarks after a change (profiles/r18_timeline_train.txt has the figures).
template <class T, bool SILU>
AUM_DEV void convp_bwd_wave(const ConvpBwdArgs& a, int wg) {
    constexpr int V = convt_vec<T, true>(), NP = V / 2, ES = (int)sizeof(T), W = CONVT_W, UB = STREAM_UB;
    const int ncb = convt_cblocks<T, true>(a.dim);
    const int cb = wg % ncb, i = wg / ncb;
    int r0, L;
    if (!train_seq(a.cu_seqlens, i, a.total, r0, L)) return;
    AumConvTmArgs sa = {};
    sa.weight = a.weight;
    sa.bias = a.bias;
    sa.dim = a.dim;
    sa.width = a.width;
    ConvtLane<T, true> ln;
    convt_lane_setup<T, true>(sa, cb, ln);
    const gbuf<T> xb = make_gbuf(row_ptr<T>(a.x, (int64_t)r0 * a.x_ts));
    const gbuf<T> gb = make_gbuf(row_ptr<T>(a.dy, (int64_t)r0 * a.dy_ts));
    const gbuf<T> dxb = make_gbuf(row_ptr<T>(a.dx, (int64_t)r0 * a.dx_ts));
    const vi coff = ln.c0 * ES;
    const int x_tb = (int)a.x_ts * ES, g_tb = (int)a.dy_ts * ES, dx_tb = (int)a.dx_ts * ES;
    const vf2 zero2 = spl2(splat(0.f)), one2 = spl2(splat(1.f));
    vf2 w2[W][NP], bias2[NP], xr[W][NP], ga[W - 1][NP], dw[W][NP], db[NP];
    AUM_UNROLL
    for (int p = 0; p < NP; ++p) {
        bias2[p] = mk2(ln.bias[2 * p], ln.bias[2 * p + 1]);
        db[p] = zero2;
        AUM_UNROLL
        for (int k = 0; k < W; ++k) {
            w2[k][p] = mk2(ln.w[k][2 * p], ln.w[k][2 * p + 1]);
            xr[k][p] = zero2;                   // xr[1 .. 3]: the last three committed inputs (zeros in front of the sequence)
            dw[k][p] = zero2;
            if (k < W - 1) ga[k][p] = zero2;    // ga[k]: what the rows so far add to dx of the committed row in xr[k + 1]
        }
    }
    int pend[W - 1] = {-1, -1, -1};             // the rows ga[0 .. 2] belong to (-1: in front of the sequence)
    auto unpack2 = [&](const convt_raw<T, true>& q, vf2 (&o)[NP]) {
        vf t[V];
        convt_unpack<T, true>(q, t);
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) o[p] = mk2(t[2 * p], t[2 * p + 1]);
    };
    auto store_dx = [&](int row, const vf2 (&v)[NP]) {
        vf o[V];
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) {
            o[2 * p] = lo2(v[p]);
            o[2 * p + 1] = hi2(v[p]);
        }
        convt_store_m<T, true>(dxb, coff, row * dx_tb, o, ln.live);
    };
    auto load_blk = [&](int itb, convt_raw<T, true> (&rx)[UB], convt_raw<T, true> (&rg)[UB]) {
        AUM_UNROLL
        for (int j = 0; j < UB; ++j) {
            const int it = itb + j < L ? itb + j : L - 1;
            rx[j] = convt_load<T, true>(xb, coff, it * x_tb);
            rg[j] = convt_load<T, true>(gb, coff, it * g_tb);
        }
    };
    auto step = [&](int it, const convt_raw<T, true>& rx, const convt_raw<T, true>& rg, bool adv) {
        vf2 xn[NP], g[NP], own[NP];
        unpack2(rx, xn);
        unpack2(rg, g);
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) {
            vf2 d = g[p];
            if (SILU) {
                vf2 pre = bias2[p];
                AUM_UNROLL
                for (int k = 0; k < W - 1; ++k) pre = vfma2(w2[k][p], xr[k + 1][p], pre);
                pre = vfma2(w2[W - 1][p], xn[p], pre);
                const vf2 sg = vsigmoid2(pre);
                d = d * (sg * vfma2(pre, one2 - sg, one2));
            }
            db[p] = db[p] + d;
            AUM_UNROLL
            for (int k = 0; k < W - 1; ++k) {
                dw[k][p] = vfma2(d, xr[k + 1][p], dw[k][p]);
                ga[k][p] = vfma2(w2[k][p], d, ga[k][p]);
            }
            dw[W - 1][p] = vfma2(d, xn[p], dw[W - 1][p]);
            own[p] = w2[W - 1][p] * d;
        }
        if (adv) {
            // the row enters the window; the oldest committed row leaves it: no later row reaches it
            if (pend[0] >= 0) store_dx(pend[0], ga[0]);
            AUM_UNROLL
            for (int p = 0; p < NP; ++p) {
                AUM_UNROLL
                for (int k = 0; k < W - 2; ++k) ga[k][p] = ga[k + 1][p];
                ga[W - 2][p] = own[p];
                AUM_UNROLL
                for (int k = 0; k < W - 1; ++k) xr[k][p] = xr[k + 1][p];
                xr[W - 1][p] = xn[p];
            }
            AUM_UNROLL
            for (int k = 0; k < W - 2; ++k) pend[k] = pend[k + 1];
            pend[W - 2] = it;
        } else {
            store_dx(it, own);                  // a peek row is in no other row's window
        }
    };
    int next_peek = a.pe;
    auto comp_blk = [&](int itb, const convt_raw<T, true> (&rx)[UB], const convt_raw<T, true> (&rg)[UB]) {
        AUM_UNROLL
        for (int j = 0; j < UB; ++j) {
            if (itb + j < L) {
                const bool pk = itb + j == next_peek;
                if (pk) next_peek += a.pe + 1;
                step(itb + j, rx[j], rg[j], !pk);
            }
        }
    };
    convt_raw<T, true> ax[UB], ag[UB], bx[UB], bg[UB];
    load_blk(0, ax, ag);
    for (int itb = 0; itb < L; itb += 2 * UB) {
        load_blk(itb + UB, bx, bg);
        comp_blk(itb, ax, ag);
        load_blk(itb + 2 * UB, ax, ag);
        comp_blk(itb + UB, bx, bg);
    }
    AUM_UNROLL
    for (int k = 0; k < W - 1; ++k)
        if (pend[k] >= 0) store_dx(pend[k], ga[k]);
    // the sequence's partial rows: dw [seq][dim][width] (the real taps of the right-aligned four), db [seq][dim]
    float* dwp = a.dw_part + (int64_t)i * a.dim * a.width;
    AUM_UNROLL
    for (int p = 0; p < NP; ++p) {
        AUM_UNROLL
        for (int k = 0; k < W; ++k) {
            const int kk = k - (W - a.width);
            if (kk >= 0) {
                gstore(dwp, (ln.c0 + 2 * p) * a.width + kk, lo2(dw[k][p]), ln.live);
                gstore(dwp, (ln.c0 + 2 * p + 1) * a.width + kk, hi2(dw[k][p]), ln.live);
            }
        }
        if (a.db_part) {
            gstore(a.db_part + (int64_t)i * a.dim, ln.c0 + 2 * p, lo2(db[p]), ln.live);
            gstore(a.db_part + (int64_t)i * a.dim, ln.c0 + 2 * p + 1, hi2(db[p]), ln.live);
        }
    }
}

}  // namespace aum
