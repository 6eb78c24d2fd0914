// stft_kernels.h -- the EPIC-Sounds frontend on the GPU: librosa-style log-mel spectrogram (one 256-thread workgroup per output
// frame) and the SpecAugment time warp of that recipe (one lane per spectrogram element).
//
// Log-mel: replaces librosa.stft(n_fft, hann(win) centred in the frame, hop, center=True, zero padding) -> |X| -> HTK mel (norm=None)
// -> log(x + eps) -> edge padding to target_length, which the reference runs on CPU DataLoader workers
// (src/epic_sounds/epic_data/audio_loader_epicsounds.py:94-156).  The magnitude of a frame does not depend on where the window sits in
// it, so the win non-zero samples are placed at the start of the frame.  The n_fft-point real DFT is one n_fft/2-point complex FFT
// of z[m] = y[2m] + i y[2m+1] (radix-2 in LDS, as fbank_kernels.h) and the usual even/odd split,
//   X[k] = E[k] + W^k O[k],  E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / 2i,  M = n_fft / 2,  W = exp(-2 pi i / n_fft).
// Time warp: spec_augment.py:346-360 with dense_image_warp's bilinear rule (:199-345); see include/aum_hip.h.
#pragma once
#include "../../include/aum_hip.h"
#include "wave.h"
#include "fbank_kernels.h"        // bit_reverse

namespace aum {

constexpr int STFT_NW = 4;                      // waves per workgroup
constexpr int STFT_THREADS = STFT_NW * WAVE;
constexpr int STFT_MAX_M = AUM_STFT_MAX_FFT / 2;        // complex FFT length
constexpr int STFT_LDS_FLOATS = 2 * STFT_MAX_M + STFT_MAX_M + 1 + 3;

// one output frame: wg = b * target_length + t
AUM_DEV void stft_logmel_frame(const AumStftArgs& p, int wg, float* lds) {
    const int b = wg / p.target_length, t = wg % p.target_length;
    float* re = lds;
    float* im = lds + STFT_MAX_M;
    float* mag = lds + 2 * STFT_MAX_M;
    int nv = p.n_valid[b];
    nv = nv < 0 ? 0 : (nv > p.n_samples ? p.n_samples : nv);
    const int frames = 1 + nv / p.hop;
    const int f = t < frames ? t : frames - 1;                  // np.pad(..., 'edge') of the frames past the clip
    const int base = f * p.hop - p.n_fft / 2 + (p.n_fft - p.win) / 2;
    const float* x = p.wave + (int64_t)b * p.wave_bs;
    const int M = p.n_fft / 2;
    int bits = 0;
    while ((1 << bits) < M) ++bits;
    // ---- windowed samples, packed two per complex value, bit-reversed store
    AUM_FOR_EACH_WAVE(w, STFT_NW) {
        for (int m0 = w * WAVE; m0 < M; m0 += STFT_THREADS) {
            const vi m = lane_id() + m0;
            const vi j0 = m * 2, j1 = m * 2 + 1;
            const vi s0 = j0 + base, s1 = j1 + base;
            const vm in0 = (j0 < p.win) && (s0 >= 0) && (s0 < nv);
            const vm in1 = (j1 < p.win) && (s1 >= 0) && (s1 < nv);
            const vf v0 = gload(x, vmax_i(s0, 0), in0) * gload(p.window, vmin_i(j0, p.win - 1), in0);
            const vf v1 = gload(x, vmax_i(s1, 0), in1) * gload(p.window, vmin_i(j1, p.win - 1), in1);
            const vi r = bit_reverse(m, bits);
            lds_write(re, r, v0);
            lds_write(im, r, v1);
        }
    }
    AUM_WG_BARRIER();
    // ---- radix-2 decimation-in-time FFT of length M; W_M^k = twiddle[2k] of the n_fft table
    for (int s = 0; s < bits; ++s) {
        const int half = 1 << s;
        AUM_FOR_EACH_WAVE(w, STFT_NW) {
            for (int j0 = w * WAVE; j0 < M / 2; j0 += STFT_THREADS) {
                const vi j = lane_id() + j0;
                const vi grp = j >> s;
                const vi pos = j - (grp << s);
                const vi i0 = (grp << (s + 1)) + pos;
                const vi i1 = i0 + half;
                const vi tk = pos * (M / half);                 // 2 * pos * (M / 2 / half): index into the n_fft table
                const vf wr = gload(p.twiddle, tk * 2, j >= 0), wi = gload(p.twiddle, tk * 2 + 1, j >= 0);
                const vf ar = lds_read(re, i0), ai = lds_read(im, i0);
                const vf br = lds_read(re, i1), bi = lds_read(im, i1);
                const vf tr = br * wr - bi * wi, ti = br * wi + bi * wr;
                lds_write(re, i0, ar + tr);
                lds_write(im, i0, ai + ti);
                lds_write(re, i1, ar - tr);
                lds_write(im, i1, ai - ti);
            }
        }
        AUM_WG_BARRIER();
    }
    // ---- even/odd split of the packed transform: |X[k]|, k = 0 .. M
    AUM_FOR_EACH_WAVE(w, STFT_NW) {
        for (int k0 = w * WAVE; k0 < M + 1; k0 += STFT_THREADS) {
            const vi k = vmin_i(lane_id() + k0, M);
            const vi ka = k & (M - 1), kb = (spl_i(M) - k) & (M - 1);
            const vf zr = lds_read(re, ka), zi = lds_read(im, ka);
            const vf cr = lds_read(re, kb), ci = splat(0.f) - lds_read(im, kb);      // conj Z[M - k]
            const vf er = (zr + cr) * 0.5f, ei = (zi + ci) * 0.5f;
            const vf orr = (zi - ci) * 0.5f, oi = (cr - zr) * 0.5f;                 // (Z - conj Z[M-k]) / 2i
            const vm last = k >= M;
            const vf wr = vsel(last, splat(-1.f), gload(p.twiddle, vmin_i(k, M - 1) * 2, !last));
            const vf wi = vsel(last, splat(0.f), gload(p.twiddle, vmin_i(k, M - 1) * 2 + 1, !last));
            const vf xr = er + (orr * wr - oi * wi), xi = ei + (orr * wi + oi * wr);
            lds_write(mag, k, vsqrt(xr * xr + xi * xi));
        }
    }
    AUM_WG_BARRIER();
    // ---- sparse mel filters, log
    float* out = p.out + (int64_t)b * p.out_bs + (int64_t)t * p.num_mel;
    AUM_FOR_EACH_WAVE(w, STFT_NW) {
        for (int m0 = w * WAVE; m0 < p.num_mel; m0 += STFT_THREADS) {
            const vi m = lane_id() + m0;
            const vm ok = m < p.num_mel;
            const vi mc = vmin_i(m, p.num_mel - 1);
            const vf startf = gload(p.mel_start_f, mc, ok), countf = gload(p.mel_count_f, mc, ok);
            const vi start = vcvt_i(startf);
            vf e = splat(0.f);
            for (int c = 0; c < p.mel_wstride; ++c) {
                const vm use = ok && (countf > (float)c);
                if (!any_lane(use)) break;
                const vi bin = vmin_i(start + c, M);
                e = vfma(gload(p.mel_w, mc * p.mel_wstride + c, use), vsel(use, lds_read(mag, bin), splat(0.f)), e);
            }
            gstore(out, m, vlog2(e + p.eps) * LN2, ok);
        }
    }
}

// time warp: STFT_NW waves of 64 elements per workgroup, element e = (b * frames + x) * num_mel + y
AUM_DEV void spec_time_warp_wg(const AumTimeWarpArgs& p, int wg) {
    const int64_t per_clip = (int64_t)p.frames * p.num_mel;
    const int64_t total = per_clip * p.batch;
    AUM_FOR_EACH_WAVE(w, STFT_NW) {
        const int64_t e0 = ((int64_t)wg * STFT_NW + w) * WAVE;
        if (e0 < total) {
            const vi le = lane_id();
            const vm ok = le < (int)(total - e0 < WAVE ? total - e0 : WAVE);
            const int b0 = (int)(e0 / per_clip);
            const vi r0 = le + (int)(e0 - (int64_t)b0 * per_clip);          // < per_clip + 64
            const vm next = r0 >= (int)per_clip;                             // the wave crosses into clip b0 + 1
            const vi b = vsel_i(next, spl_i(b0 + 1), spl_i(b0));
            const vi r = vsel_i(next, r0 - (int)per_clip, r0);
            const vi x = r / p.num_mel, y = r - x * p.num_mel;
            const vi bt = vmin_i(b, p.batch - 1) * AUM_TIME_WARP_COLS;
            const vf cy = gload(p.table, bt, ok), cx = gload(p.table, bt + 1, ok), ww = gload(p.table, bt + 2, ok);
            const vf v0 = gload(p.table, bt + 3, ok), v1 = gload(p.table, bt + 4, ok), v2 = gload(p.table, bt + 5, ok);
            const vf xn = gload(p.table, bt + 6, ok), yn = gload(p.table, bt + 7, ok);
            const vf qy = vcvt_f(y), qx = vcvt_f(x);
            // the spline: phi(r) w + [y x 1] v, the reference's operation order (apply_interpolation, cross_squared_distance_matrix, phi)
            const vf rr = (xn - (qy * cy + qx * cx) * 2.f) + yn;
            const vf phi = (rr * 0.5f) * (vlog2(vmax(rr, splat(1e-10f))) * LN2);
            const vf flow = phi * ww + ((qy * v0 + qx * v1) + v2);
            // bilinear sample at (y, x - flow) (interpolate_bilinear: floor clamped to [0, size - 2], weight clamped to [0, 1])
            const vf sx = qx - flow;
            const vf fx = vmin(vmax(splat(0.f), vfloor(sx)), splat((float)(p.frames - 2)));
            const vf fy = vmin(vmax(splat(0.f), vfloor(qy)), splat((float)(p.num_mel - 2)));
            const vf ax = vmin(vmax(splat(0.f), sx - fx), splat(1.f));
            const vf ay = vmin(vmax(splat(0.f), qy - fy), splat(1.f));
            const vi ix = vcvt_i(fx), iy = vcvt_i(fy);
            const vi bc = vmin_i(b, p.batch - 1);
            const vi o00 = ix * p.num_mel + iy;
            const float* src = p.in;
            auto at = [&](vi o) {               // in[b][o] with a 64-bit clip offset
                vf v = splat(0.f);
                for (int q = 0; q < 2; ++q) {   // the two clips a wave can touch
                    const int bq = b0 + q < p.batch ? b0 + q : p.batch - 1;
                    const vm sel = ok && (bc == bq);
                    if (any_lane(sel)) v = vsel(sel, gload(src + (int64_t)bq * p.in_bs, o, sel), v);
                }
                return v;
            };
            const vf tl = at(o00), tr = at(o00 + p.num_mel), bl = at(o00 + 1), br = at(o00 + p.num_mel + 1);
            const vf it = ax * (tr - tl) + tl;
            const vf ib = ax * (br - bl) + bl;
            const vf v = ay * (ib - it) + it;
            for (int q = 0; q < 2; ++q) {
                const int bq = b0 + q < p.batch ? b0 + q : p.batch - 1;
                const vm sel = ok && (bc == bq);
                if (any_lane(sel)) gstore(p.out + (int64_t)bq * p.out_bs, r, v, sel);
            }
        }
    }
}

}  // namespace aum
