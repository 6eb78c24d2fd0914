// stream_prefill_kernels.h -- PACKED PREFILL: the backlogs of several streaming sessions through the time-parallel conv and the state in /
// state out scan of the offline forward in one launch each (include/aum_hip.h: aum_conv1d_tm_prefill_var, aum_scan_tm_fwd_state_var).
// Packed rows, cu_seqlens, state_indices and the no-op rule are those of stream_tm_kernels.h (stream_seq); the steps are those of
// conv_tm_kernels.h (convt_fwd_wave) and scan_tm_kernels.h (scant_fwd_run PHASE 0 / 3, called as they are).  A session longer than the
// max_len the host sized the grid with is a no-op as well.
//
// CONV (convp_var_wave).  Unit = (session, chunk of convt_tc(len_i) <= 64 steps, block of 64 * V channels), channel block fastest; the
// grid holds convt_chunks(max_len) chunks per session and the chunks past a session's own count return at once.  The step is
// convt_fwd_wave's: y = act(bias + w0 x[t-3] + w1 x[t-2] + w2 x[t-1] + w3 x[t]) on channel pairs, the window a ring of four register
// rows, two blocks of eight rows in flight, requests clamped to the chunk's last row -- a session's rows are never left, in either
// direction.  The conv is not recurrent: where the chunk boundaries fall does not change a bit.
//   window read   the rows before a session's first row are conv_state[row, :, 1:], read as fp32 straight into the ring (no rounding to
//                 the row dtype, no [window ; x] copy).  Only the wave of chunk 0 needs them; every later chunk's window is three rows
//                 of x (a second chunk exists only behind more than 64 rows).
//   window write  afterwards conv_state[row] holds the session's last `width` inputs; fewer rows than `width`: the old entries shift.
//   WHICH WAVE, AND WHY THE ORDER HOLDS: the wave of CHUNK 0 of a (session, channel block) is the only wave of the launch that touches
//                 that part of the session's cache row -- it reads the old window ahead of its first step and, BEHIND its last step,
//                 fetches the session's last `width` rows of x (clamped to row 0) and, for a session shorter than `width`, the old
//                 entries that survive once more, and only then stores the new window.  Reads and writes of the row are therefore one
//                 wave's own accesses in program order: every stored value is either data the loads in front of the stores returned
//                 (a true dependency) or a row of x, and all loads of old entries are issued before the first store.  No other wave --
//                 not the later chunks of the session, not another session (the host refuses two sessions on one row) -- reads or
//                 writes it, so there is no second launch for the write-back and no ordering between waves to rely on.
//
// SCAN (scant_fwd_state_var, scant_seg_fwd_state_var).  scant_fwd_run addresses a row as `b * X_bs + t * X_ts` and takes its length from
// p.len, so every item runs it on a LOCAL COPY of the launch's argument struct with len := the session's length, called with b := the
// session's first packed row (the launcher sets X_bs := X_ts): scant_fwd_run itself is untouched and sees an ordinary row.
//   staging       the 8-step block staging of scant_fwd_run clamps the rows of a ragged block into [it0, it1) of the item and masks
//                 its stores, and blocks inside the range are whole: with the row base at the session's first row it never STORES
//                 outside the session's rows, and it never reads outside them either -- so every read lands in rows that exist
//                 (inside [0, total) of the packed operands) whatever the neighbours hold.
//   uncut         one wave per (session, 64 channels): x <- state[row], the session's rows, state[row] <- x, by the same lane.
//   cut           every session into nranges = ceil(max_len / range_len) ranges of range_len steps (a multiple of the checkpoint block);
//                 item = (session, 64 channels, range).  Session i has nr_i = ceil(len_i / range_len) ranges that hold steps; the
//                 ranges past its end are empty: their waves return and the state is handed through untouched, because it is the
//                 wave of range nr_i - 1 that stores state[row] behind the session's last step.
//                 carry launch   ranges 0 .. nr_i - 2 from a zero state: exit state X_s and decay product P_s (PHASE 3) into the
//                                session's carry slots; the wave of range nranges - 1 parks state[row] in the X rows of slot
//                                nranges - 1, which no carry uses (nr_i - 1 <= nranges - 1 is the last range that runs).
//                 main launch    range s starts from P_{s-1} ( ... (P_0 entry + X_0) ... ) + X_{s-1} and runs PHASE 0.
//                 state[row] is read by the carry launch only and written by the main launch only: the stream orders them.
//                 A session whose own cut (aum_scan_tm_fwd_state with segments = nr_i) has ranges of range_len steps gets that call's
//                 bits: the same ranges, the same carries composed in the same order.
#pragma once
#include "stream_tm_kernels.h"

namespace aum {

// ---- conv ---------------------------------------------------------------------------------------
template <class T, bool SILU>
AUM_DEV void convp_var_wave(const AumConvTmPrefillVarArgs& a, int wg) {
    constexpr int V = convt_vec<T, false>(), NP = V / 2, ES = (int)sizeof(T), W = CONVT_W;
    const int ncb = convt_cblocks<T, false>(a.dim), nchm = convt_chunks<false>(a.max_len);
    const int cb = wg % ncb, ch = (wg / ncb) % nchm, i = wg / (ncb * nchm);
    int r0, L, row;
    if (!stream_seq(a.cu_seqlens, a.state_indices, i, a.total, a.nrows, r0, L, row) || L > a.max_len) return;
    if (ch >= convt_chunks<false>(L)) return;
    AumConvTmArgs s = {};
    s.weight = a.weight;
    s.bias = a.bias;
    s.dim = a.dim;
    s.width = a.width;
    ConvtLane<T, false> ln;
    convt_lane_setup<T, false>(s, cb, ln);
    const gbuf<T> xb = make_gbuf(row_ptr<T>(a.x, (int64_t)r0 * a.x_ts));
    const gbuf<T> yb = make_gbuf(row_ptr<T>(a.y, (int64_t)r0 * a.y_ts));
    float* win = a.conv_state + (int64_t)row * a.dim * a.width;
    const vi coff = ln.c0 * ES;
    const int x_tb = (int)a.x_ts * ES, y_tb = (int)a.y_ts * ES;
    const int tc = convt_tc<false>(L);
    const int it0 = ch * tc, it1 = it0 + tc < L ? it0 + tc : L;
    vf2 w2[W][NP], bias2[NP], xr[W][NP];
    AUM_UNROLL
    for (int p = 0; p < NP; ++p) {
        bias2[p] = mk2(ln.bias[2 * p], ln.bias[2 * p + 1]);
        AUM_UNROLL
        for (int k = 0; k < W; ++k) {
            w2[k][p] = mk2(ln.w[k][2 * p], ln.w[k][2 * p + 1]);
            xr[k][p] = spl2(splat(0.f));
        }
    }
    auto unpack2 = [&](const convt_raw<T, false>& q, vf2 (&o)[NP]) {
        vf t[V];
        convt_unpack<T, false>(q, t);
        AUM_UNROLL
        for (int p = 0; p < NP; ++p) o[p] = mk2(t[2 * p], t[2 * p + 1]);
    };
    // the window before the chunk: steps it0 - 3 .. it0 - 1.  Chunk 0: conv_state[j] is input j - width, so step -3 + k is entry
    // width - 3 + k, of which entries 1 .. width - 1 are read (entry 0 meets no tap of this call; older steps are zero)
    AUM_UNROLL
    for (int k = 0; k < W - 1; ++k) {
        if (ch == 0) {
            const int j = a.width - (W - 1) + k;
            if (j >= 1) {
                AUM_UNROLL
                for (int p = 0; p < NP; ++p) xr[k][p] = mk2(gload_u(win, (ln.c0 + 2 * p) * a.width + j), gload_u(win, (ln.c0 + 2 * p + 1) * a.width + j));
            }
        } else {
            unpack2(convt_load<T, false>(xb, coff, (it0 - (W - 1) + k) * x_tb), xr[k]);       // it0 >= 33: these rows are the session's
        }
    }
    const bool all_live = a.dim % (WAVE * V) == 0;
    auto load_blk = [&](int itb, convt_raw<T, false> (&raw)[CONVT_UB]) {
        AUM_UNROLL
        for (int j = 0; j < CONVT_UB; ++j) {
            const int it = itb + j < it1 ? itb + j : it1 - 1;
            raw[j] = convt_load<T, false>(xb, coff, it * x_tb);
        }
    };
    static_assert(CONVT_UB % CONVT_W == 0, "a block returns the ring to its phase");
    auto comp_blk = [&](int itb, const convt_raw<T, false> (&raw)[CONVT_UB]) {
        AUM_UNROLL
        for (int j = 0; j < CONVT_UB; ++j) {
            if (itb + j < it1) {
                auto X = [&](int k) -> vf2 (&)[NP] { return xr[(k + j) & (W - 1)]; };
                unpack2(raw[j], X(W - 1));
                vf y[V];
                AUM_UNROLL
                for (int p = 0; p < NP; ++p) {
                    vf2 acc = bias2[p];
                    AUM_UNROLL
                    for (int k = 0; k < W; ++k) acc = vfma2(w2[k][p], X(k)[p], acc);
                    if (SILU) acc = acc * vsigmoid2(acc);
                    y[2 * p] = lo2(acc);
                    y[2 * p + 1] = hi2(acc);
                }
                if (all_live) convt_store<T, false>(yb, coff, (itb + j) * y_tb, y);
                else convt_store_m<T, false>(yb, coff, (itb + j) * y_tb, y, ln.live);
            }
        }
    };
    {
        convt_raw<T, false> ra[CONVT_UB], rb[CONVT_UB];
        load_blk(it0, ra);
        for (int itb = it0; itb < it1; itb += 2 * CONVT_UB) {
            load_blk(itb + CONVT_UB, rb);
            comp_blk(itb, ra);
            load_blk(itb + 2 * CONVT_UB, ra);
            comp_blk(itb + CONVT_UB, rb);
        }
    }
    if (ch != 0) return;
    // the new window, by the wave that read the old one: slot i (right-aligned: real from W - width) is input L - W + i -- a row of x,
    // or for a session shorter than the window the old entry i - (W - width) + L.  All loads first, then the stores.
    vf2 nw[W][NP];
    AUM_UNROLL
    for (int k = 0; k < W; ++k) {
        const int t = L - W + k, j = k - (W - a.width);
        unpack2(convt_load<T, false>(xb, coff, (t > 0 ? t : 0) * x_tb), nw[k]);
        if (t < 0 && j >= 0) {
            AUM_UNROLL
            for (int p = 0; p < NP; ++p)
                nw[k][p] = mk2(gload_u(win, (ln.c0 + 2 * p) * a.width + (j + L)), gload_u(win, (ln.c0 + 2 * p + 1) * a.width + (j + L)));
        }
    }
    AUM_UNROLL
    for (int k = 0; k < W; ++k) {
        const int j = k - (W - a.width);
        if (j >= 0) {
            AUM_UNROLL
            for (int p = 0; p < NP; ++p) {
                gstore(win, (ln.c0 + 2 * p) * a.width + j, lo2(nw[k][p]), ln.live);
                gstore(win, (ln.c0 + 2 * p + 1) * a.width + j, hi2(nw[k][p]), ln.live);
            }
        }
    }
}

// ---- scan ---------------------------------------------------------------------------------------
// what the items of one launch read next to the argument struct (p: X_bs == X_ts, batch == nseq, len unused)
struct ScanTVar {
    const int32_t *cu_seqlens, *state_indices;
    float* state;          // (nrows, dim, N) fp32, the named rows advanced in place
    int total, nseq, nrows, max_len;
};

// workgroup = four waves, four (session, channel group) units
template <class T, bool SP, bool HAS_Z>
AUM_DEV void scant_fwd_state_var(const AumScanTmFwdArgs& p, const ScanTVar& v, int wg, float* lds) {
    constexpr int N = SCANT_N;
    constexpr int NW = SCANT_NW;
    const int gpb = p.dim / WAVE;
    const int units = v.nseq * gpb;
    vf2 x[AUM_PER_WAVE(NW)][N / 2];
    AUM_FOR_EACH_WAVE(w, NW) {
        const int unit = wg * NW + w;
        if (unit < units) {
            const int i = unit / gpb, e0 = (unit % gpb) * WAVE;
            int r0, len, row;
            if (stream_seq(v.cu_seqlens, v.state_indices, i, v.total, v.nrows, r0, len, row) && len <= v.max_len) {
                AumScanTmFwdArgs q = p;
                q.len = len;
                const vi ec = lane_id() + e0;
                float* st = v.state + (int64_t)row * p.dim * N;
                scant_state_load<N>(st, ec, x[AUM_W(w)]);
                scant_fwd_run<T, N, 0, SP, HAS_Z, false>(q, r0, e0, 0, 0, 1, 0, len, q.A, 1.f, x[AUM_W(w)], lds + w * scant_lds_wave_floats<T>());
                scant_state_store<N>(st, ec, x[AUM_W(w)]);
            }
        }
    }
}

// workgroup = four independent waves; item = ((session * groups) + channel group) * nseg + range.  sg: nseg = nranges, seg_len =
// range_len, carry [nseq][nseg][2][N][dim].  PHASE 3: the carry launch; PHASE 0: the main launch.
template <class T, int PHASE, bool SP, bool HAS_Z>
AUM_DEV void scant_seg_fwd_state_var(const AumScanTmFwdArgs& p, const ScanTSeg& sg, const ScanTVar& v, int wg, float* lds) {
    static_assert(PHASE == 0 || PHASE == 3, "carry launch or main launch");
    constexpr int N = SCANT_N;
    constexpr int NW = SCANT_NW;
    const int gpb = p.dim / WAVE;
    const int items = v.nseq * gpb * sg.nseg;
    vf2 x[AUM_PER_WAVE(NW)][N / 2], P[AUM_PER_WAVE(NW)][N / 2];
    AUM_FOR_EACH_WAVE(w, NW) {
        const int item = wg * NW + w;
        if (item < items) {
            const int s = item % sg.nseg, unit = item / sg.nseg;
            const int i = unit / gpb, e0 = (unit % gpb) * WAVE;
            int r0, len, row;
            if (stream_seq(v.cu_seqlens, v.state_indices, i, v.total, v.nrows, r0, len, row) && len <= v.max_len) {
                const int last = (len + sg.seg_len - 1) / sg.seg_len - 1;       // the last range that holds steps (<= nseg - 1)
                const int it0 = s * sg.seg_len < len ? s * sg.seg_len : len;
                const int it1 = it0 + sg.seg_len < len ? it0 + sg.seg_len : len;
                const vi ec = lane_id() + e0;
                float* cb = sg.carry + (int64_t)i * sg.nseg * (2 * N) * p.dim;
                float* entry = cb + (int64_t)(sg.nseg - 1) * (2 * N) * p.dim + (int64_t)N * p.dim;      // X rows of the last slot
                float* lw = lds + w * scant_lds_wave_floats<T>();
                float* st = v.state + (int64_t)row * p.dim * N;
                AumScanTmFwdArgs q = p;
                q.len = len;
                if (PHASE == 3) {
                    if (s == sg.nseg - 1) {
                        scant_state_load<N>(st, ec, x[AUM_W(w)]);
                        AUM_UNROLL
                        for (int n = 0; n < N; ++n)
                            gstore(entry + (int64_t)n * p.dim, ec, (n & 1) ? hi2(x[AUM_W(w)][n >> 1]) : lo2(x[AUM_W(w)][n >> 1]), ec >= 0);
                    } else if (s < last) {
                        AUM_UNROLL
                        for (int j = 0; j < N / 2; ++j) {
                            x[AUM_W(w)][j] = spl2(splat(0.f));
                            P[AUM_W(w)][j] = spl2(splat(1.f));
                        }
                        scant_fwd_run<T, N, 3, SP, false, false>(q, r0, e0, 0, 0, 1, it0, it1, q.A, 1.f, x[AUM_W(w)], lw, nullptr, P[AUM_W(w)]);
                        float* cs = cb + (int64_t)s * (2 * N) * p.dim;
                        AUM_UNROLL
                        for (int n = 0; n < N; ++n) {
                            gstore(cs + (int64_t)n * p.dim, ec, (n & 1) ? hi2(P[AUM_W(w)][n >> 1]) : lo2(P[AUM_W(w)][n >> 1]), ec >= 0);
                            gstore(cs + (int64_t)(N + n) * p.dim, ec, (n & 1) ? hi2(x[AUM_W(w)][n >> 1]) : lo2(x[AUM_W(w)][n >> 1]), ec >= 0);
                        }
                    }
                } else if (s <= last) {
                    AUM_UNROLL
                    for (int j = 0; j < N / 2; ++j)
                        x[AUM_W(w)][j] = mk2(gload_u(entry + (int64_t)(2 * j) * p.dim, ec), gload_u(entry + (int64_t)(2 * j + 1) * p.dim, ec));
                    for (int sp = 0; sp < s; ++sp) {
                        const float* cs = cb + (int64_t)sp * (2 * N) * p.dim;
                        AUM_UNROLL
                        for (int j = 0; j < N / 2; ++j) {
                            const vf2 pj = mk2(gload_u(cs + (int64_t)(2 * j) * p.dim, ec), gload_u(cs + (int64_t)(2 * j + 1) * p.dim, ec));
                            const vf2 xj = mk2(gload_u(cs + (int64_t)(N + 2 * j) * p.dim, ec), gload_u(cs + (int64_t)(N + 2 * j + 1) * p.dim, ec));
                            x[AUM_W(w)][j] = vfma2(pj, x[AUM_W(w)][j], xj);
                        }
                    }
                    scant_fwd_run<T, N, 0, SP, HAS_Z, false>(q, r0, e0, 0, 0, 1, it0, it1, q.A, 1.f, x[AUM_W(w)], lw);
                    if (s == last) scant_state_store<N>(st, ec, x[AUM_W(w)]);
                }
            }
        }
    }
}

}  // namespace aum
