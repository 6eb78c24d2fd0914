// aum_api_tm.inc -- C-ABI entry points, kernel entries and launchers of the time-serial token-major scan (scan_tm_kernels.h), the
// token-major conv and the streaming kernels.  Launches, LDS and flag / dtype dispatch as in aum_api.inc: AUM_LAUNCH, Lds<>, with_bool /
// with_int / by_dtype of launch.h.
// Included at the end of aum_api.inc.  AUM_API_PART 5 / 6 (with AUM_DTYPE_ONLY) are the forward / backward kernel objects of the
// device library; part 3 holds the extern "C" surface; part 0 (the lane-array test build) holds everything.
#include "scan_tm_kernels.h"
#include "conv_tm_kernels.h"
#include "stream_tm_kernels.h"
#include "stream_train_kernels.h"
#include "stream_block_kernels.h"
#include "stream_prefill_kernels.h"

namespace aum {

#ifndef AUM_SCANT_FWD_MINW
#define AUM_SCANT_FWD_MINW 3      // waves per SIMD the forward is compiled for (<= 168 VGPRs): B = 64, E = 1536 is exactly 3 per SIMD
#endif

int scan_tm_fwd_f32(const AumScanTmFwdArgs& a, aum_stream_t s);
int scan_tm_fwd_bf16(const AumScanTmFwdArgs& a, aum_stream_t s);
int scan_tm_fwd_f16(const AumScanTmFwdArgs& a, aum_stream_t s);
int scan_tm_bwd_f32(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s);
int scan_tm_bwd_bf16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s);
int scan_tm_bwd_f16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s);
// time-segmented launches (scant_seg_fwd / scant_seg_bwd): one launch of `phase` over the directions sg names
int scan_tm_seg_fwd_f32(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s);
int scan_tm_seg_fwd_bf16(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s);
int scan_tm_seg_fwd_f16(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s);
// state in / state out (scant_fwd_state; sg != nullptr: one launch of `phase` 3 or 0 of scant_seg_fwd_state)
int scan_tm_fwd_state_f32(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s);
int scan_tm_fwd_state_bf16(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s);
int scan_tm_fwd_state_f16(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s);
// the same on packed sessions (scant_fwd_state_var; sg != nullptr: one launch of `phase` 3 or 0 of scant_seg_fwd_state_var)
int scan_tm_fwd_state_var_f32(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s);
int scan_tm_fwd_state_var_bf16(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s);
int scan_tm_fwd_state_var_f16(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s);
int scan_tm_seg_bwd_f32(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s);
int scan_tm_seg_bwd_bf16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s);
int scan_tm_seg_bwd_f16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s);

// workspace of the backward (floats): dB/dC partial rows, then the per-(direction, batch entry) partials of dA, dD, ddelta_bias
struct ScanTWs { int64_t dbc, dA, dD, dbias, carry, total, trace; int nparts, ndir; };
// nseg > 1 (time segments): batch * nseg rows of dA / dD / ddelta_bias partials per direction, and `carry` holds the adjoint carries
static ScanTWs scant_ws_layout(int batch, int dim, int len, int dstate, bool bidir, int nseg = 1) {
    ScanTWs w;
    w.ndir = bidir ? 2 : 1;
    w.nparts = dim / WAVE * w.ndir;
    w.dbc = 0;
    w.dA = w.dbc + (int64_t)batch * len * w.nparts * 2 * dstate;
    w.dD = w.dA + (int64_t)w.ndir * batch * nseg * dstate * dim;
    w.dbias = w.dD + (int64_t)w.ndir * batch * nseg * dim;
    w.carry = w.dbias + (int64_t)w.ndir * batch * nseg * dim;
    if (nseg > 1) w.total = w.carry + scant_seg_carry_floats(batch, dim, nseg, bidir);
    else w.total = w.carry + (bidir ? (int64_t)scant_bwd_wgs<true>(batch * (dim / WAVE)) * 2 * (2 * dstate + 2) * WAVE : 0);
    w.trace = 0;
#ifdef AUM_SCANT_TRACE
    w.trace = (w.total + 1) / 2 * 2;
    w.total = w.trace + (int64_t)(bidir ? scant_bwd_wgs<true>(batch * (dim / WAVE)) : scant_bwd_wgs<false>(batch * (dim / WAVE))) * SCANT_NW * 16 * 2;
#endif
    return w;
}

// the LDS of every forward / backward kernel of scan_tm_kernels.h
template <class T> using ScanTFwdLds = Lds<float, SCANT_NW * scant_lds_wave_floats<T>()>;
template <class T> using ScanTBwdLds = Lds<float, SCANT_NW * scant_bwd_lds_wave_floats<T>()>;
#if AUM_API_PART == 5 || AUM_API_PART == 0
#ifndef AUM_EMU
template <class T, bool SP, bool HAS_Z, bool HAS_PRE, bool BIDIR>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_fwd(AumScanTmFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
#ifdef AUM_SCANT_TRACE      // tools/tm_trace.py builds only: where and when every wave ran (a.ckpt is the trace buffer: 12 x uint64 per wave)
    unsigned long long* tr = reinterpret_cast<unsigned long long*>(a.ckpt) + ((size_t)blockIdx.x * SCANT_NW + threadIdx.x / 64) * 12;
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
    a.ckpt = nullptr;
    unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    scant_fwd<T, SP, HAS_Z, HAS_PRE, BIDIR>(a, (int)blockIdx.x, lds, tacc);
    if ((threadIdx.x & 63) == 0) {
        tr[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_REG_HW_ID
        tr[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // HW_REG_XCC_ID
        tr[2] = t_begin;
        tr[3] = __builtin_amdgcn_s_memrealtime();
        for (int k = 0; k < 8; ++k) tr[4 + k] = tacc[k];          // shader-clock cycles: prologue, request, steps, flush, park
    }
#else
    scant_fwd<T, SP, HAS_Z, HAS_PRE, BIDIR>(a, (int)blockIdx.x, lds);
#endif
}
#endif
template <class T, bool SP, bool HAS_Z, bool HAS_PRE, bool BIDIR> static int launch_scant_fwd(const AumScanTmFwdArgs& a, aum_stream_t s) {
    constexpr int UPW = scant_units_per_wg<BIDIR>();
    const int grid = (a.batch * (a.dim / WAVE) + UPW - 1) / UPW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_fwd<T, SP, HAS_Z, HAS_PRE, BIDIR>), (scant_fwd<T, SP, HAS_Z, HAS_PRE, BIDIR>(a, wg, lds)), a);
}
template <class T> static int scan_tm_fwd_t(const AumScanTmFwdArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) { return with_bool(a.z != nullptr, [&](auto hz) {
        return with_bool(a.out_pre != nullptr, [&](auto pre) { return with_bool(a.A_b != nullptr, [&](auto bidir) {
            return launch_scant_fwd<T, sp, hz, pre, bidir>(a, s); }); }); }); });
}
#ifndef AUM_EMU
template <class T, int PHASE, bool SP, bool HAS_Z, bool HAS_PRE>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_seg_fwd(AumScanTmFwdArgs a, ScanTSeg sg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
    scant_seg_fwd<T, PHASE, SP, HAS_Z, HAS_PRE>(a, sg, (int)blockIdx.x, lds);
}
#endif
template <class T, int PHASE, bool SP, bool HAS_Z, bool HAS_PRE> static int launch_scant_seg_fwd(const AumScanTmFwdArgs& a, const ScanTSeg& sg, aum_stream_t s) {
    const int grid = (a.batch * (a.dim / WAVE) * sg.nseg * sg.ndl + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_seg_fwd<T, PHASE, SP, HAS_Z, HAS_PRE>), (scant_seg_fwd<T, PHASE, SP, HAS_Z, HAS_PRE>(a, sg, wg, lds)), a, sg);
}
template <class T> static int scan_tm_seg_fwd_t(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s) {
    // phase 3 (carries): no z, no pre-gate copy; phase 4 (adjoint carries): no pre-gate copy; phases 0 - 2: every form
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        if (phase == 3) return launch_scant_seg_fwd<T, 3, sp, false, false>(a, sg, s);
        return with_bool(a.z != nullptr, [&](auto hz) {
            if (phase == 4) return launch_scant_seg_fwd<T, 4, sp, hz, false>(a, sg, s);
            return with_bool(a.out_pre != nullptr, [&](auto pre) {
                return with_int<0, 1, 2>(phase, [&](auto ph) { return launch_scant_seg_fwd<T, ph, sp, hz, pre>(a, sg, s); }); });
        });
    });
}
#ifndef AUM_EMU
template <class T, bool SP, bool HAS_Z>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_fwd_state(AumScanTmFwdArgs a, ScanTState st) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
    scant_fwd_state<T, SP, HAS_Z>(a, st, (int)blockIdx.x, lds);
}
template <class T, int PHASE, bool SP, bool HAS_Z>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_seg_fwd_state(AumScanTmFwdArgs a, ScanTSeg sg, ScanTState st) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
    scant_seg_fwd_state<T, PHASE, SP, HAS_Z>(a, sg, st, (int)blockIdx.x, lds);
}
#endif
template <class T, bool SP, bool HAS_Z> static int launch_scant_fwd_state(const AumScanTmFwdArgs& a, const ScanTState& st, aum_stream_t s) {
    const int grid = (a.batch * (a.dim / WAVE) + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_fwd_state<T, SP, HAS_Z>), (scant_fwd_state<T, SP, HAS_Z>(a, st, wg, lds)), a, st);
}
template <class T, int PHASE, bool SP, bool HAS_Z>
static int launch_scant_seg_fwd_state(const AumScanTmFwdArgs& a, const ScanTSeg& sg, const ScanTState& st, aum_stream_t s) {
    const int grid = (a.batch * (a.dim / WAVE) * sg.nseg + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_seg_fwd_state<T, PHASE, SP, HAS_Z>), (scant_seg_fwd_state<T, PHASE, SP, HAS_Z>(a, sg, st, wg, lds)), a, sg, st);
}
template <class T> static int scan_tm_fwd_state_t(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s) {
    // segmented: phase 3 (carries, no z) and phase 0 only
    if (sg && phase != 3 && phase != 0) return AUM_E_UNSUPPORTED;
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        if (sg && phase == 3) return launch_scant_seg_fwd_state<T, 3, sp, false>(a, *sg, st, s);
        return with_bool(a.z != nullptr, [&](auto hz) {
            return sg ? launch_scant_seg_fwd_state<T, 0, sp, hz>(a, *sg, st, s) : launch_scant_fwd_state<T, sp, hz>(a, st, s);
        });
    });
}
#ifndef AUM_EMU
template <class T, bool SP, bool HAS_Z>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_fwd_state_var(AumScanTmFwdArgs a, ScanTVar v) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
    scant_fwd_state_var<T, SP, HAS_Z>(a, v, (int)blockIdx.x, lds);
}
template <class T, int PHASE, bool SP, bool HAS_Z>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_FWD_MINW) void k_scant_seg_fwd_state_var(AumScanTmFwdArgs a, ScanTSeg sg, ScanTVar v) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTFwdLds<T>::n];
    scant_seg_fwd_state_var<T, PHASE, SP, HAS_Z>(a, sg, v, (int)blockIdx.x, lds);
}
#endif
template <class T, bool SP, bool HAS_Z> static int launch_scant_fwd_state_var(const AumScanTmFwdArgs& a, const ScanTVar& v, aum_stream_t s) {
    const int grid = (v.nseq * (a.dim / WAVE) + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_fwd_state_var<T, SP, HAS_Z>), (scant_fwd_state_var<T, SP, HAS_Z>(a, v, wg, lds)), a, v);
}
template <class T, int PHASE, bool SP, bool HAS_Z>
static int launch_scant_seg_fwd_state_var(const AumScanTmFwdArgs& a, const ScanTSeg& sg, const ScanTVar& v, aum_stream_t s) {
    const int grid = (v.nseq * (a.dim / WAVE) * sg.nseg + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTFwdLds<T>{}), (k_scant_seg_fwd_state_var<T, PHASE, SP, HAS_Z>), (scant_seg_fwd_state_var<T, PHASE, SP, HAS_Z>(a, sg, v, wg, lds)), a, sg, v);
}
template <class T> static int scan_tm_fwd_state_var_t(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s) {
    // segmented: phase 3 (carries, no z) and phase 0 only
    if (sg && phase != 3 && phase != 0) return AUM_E_UNSUPPORTED;
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        if (sg && phase == 3) return launch_scant_seg_fwd_state_var<T, 3, sp, false>(a, *sg, v, s);
        return with_bool(a.z != nullptr, [&](auto hz) {
            return sg ? launch_scant_seg_fwd_state_var<T, 0, sp, hz>(a, *sg, v, s) : launch_scant_fwd_state_var<T, sp, hz>(a, v, s);
        });
    });
}
#if AUM_HAS_DTYPE(0)
int scan_tm_fwd_f32(const AumScanTmFwdArgs& a, aum_stream_t s) { return scan_tm_fwd_t<float>(a, s); }
int scan_tm_seg_fwd_f32(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_fwd_t<float>(a, sg, phase, s); }
int scan_tm_fwd_state_f32(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_t<float>(a, st, sg, phase, s); }
int scan_tm_fwd_state_var_f32(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_var_t<float>(a, v, sg, phase, s); }
#endif
#if AUM_HAS_DTYPE(1)
int scan_tm_fwd_bf16(const AumScanTmFwdArgs& a, aum_stream_t s) { return scan_tm_fwd_t<bf16_t>(a, s); }
int scan_tm_seg_fwd_bf16(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_fwd_t<bf16_t>(a, sg, phase, s); }
int scan_tm_fwd_state_bf16(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_t<bf16_t>(a, st, sg, phase, s); }
int scan_tm_fwd_state_var_bf16(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_var_t<bf16_t>(a, v, sg, phase, s); }
#endif
#if AUM_HAS_DTYPE(2)
int scan_tm_fwd_f16(const AumScanTmFwdArgs& a, aum_stream_t s) { return scan_tm_fwd_t<f16_t>(a, s); }
int scan_tm_seg_fwd_f16(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_fwd_t<f16_t>(a, sg, phase, s); }
int scan_tm_fwd_state_f16(const AumScanTmFwdArgs& a, const ScanTState& st, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_t<f16_t>(a, st, sg, phase, s); }
int scan_tm_fwd_state_var_f16(const AumScanTmFwdArgs& a, const ScanTVar& v, const ScanTSeg* sg, int phase, aum_stream_t s) { return scan_tm_fwd_state_var_t<f16_t>(a, v, sg, phase, s); }
#endif
#endif

#ifndef AUM_SCANT_BWD_MINW
#define AUM_SCANT_BWD_MINW 2      // 256 VGPRs: the pass keeps B, C, a and w of eight steps in registers
#endif
#if AUM_API_PART == 6 || AUM_API_PART == 0
#ifndef AUM_EMU
template <class T, int SP, bool HAS_Z, bool BIDIR>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_BWD_MINW) void k_scant_bwd(AumScanTmBwdArgs a, ScanTBwdOut wo) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTBwdLds<T>::n];
#ifdef AUM_SCANT_TRACE      // tools/tm_trace.py builds only: 16 x uint64 per wave behind the partials of the workspace
    unsigned long long* tr = wo.trace + ((size_t)blockIdx.x * SCANT_NW + threadIdx.x / 64) * 16;
    const unsigned long long t_begin = __builtin_amdgcn_s_memrealtime();
    unsigned long long tacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    scant_bwd<T, SP, HAS_Z, BIDIR>(a, wo, (int)blockIdx.x, lds, tacc);
    if ((threadIdx.x & 63) == 0) {
        tr[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_REG_HW_ID
        tr[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);      // HW_REG_XCC_ID
        tr[2] = t_begin;
        tr[3] = __builtin_amdgcn_s_memrealtime();
        for (int k = 0; k < 12; ++k) tr[4 + k] = tacc[k];
    }
#else
    scant_bwd<T, SP, HAS_Z, BIDIR>(a, wo, (int)blockIdx.x, lds);
#endif
}
#endif
template <class T, int SP, bool HAS_Z, bool BIDIR> static int launch_scant_bwd(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s) {
    const int grid = scant_bwd_wgs<BIDIR>(a.batch * (a.dim / WAVE));
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTBwdLds<T>{}), (k_scant_bwd<T, SP, HAS_Z, BIDIR>), (scant_bwd<T, SP, HAS_Z, BIDIR>(a, wo, wg, lds)), a, wo);
}
template <class T> static int scan_tm_bwd_t(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s) {
    if (a.flags & AUM_SCAN_DELTA_ACTIVATED) {       // built for the product path only: 16-bit activations with z (scan_tm_bwd_any checks)
        if constexpr (sizeof(T) == 2)
            return with_bool(a.A_b != nullptr, [&](auto bidir) { return launch_scant_bwd<T, SCANT_SP_ACT, true, bidir>(a, wo, s); });
        return AUM_E_UNSUPPORTED;
    }
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) { return with_bool(a.z != nullptr, [&](auto hz) {
        return with_bool(a.A_b != nullptr, [&](auto bidir) { return launch_scant_bwd<T, sp ? SCANT_SP_IN : SCANT_SP_NONE, hz, bidir>(a, wo, s); }); }); });
}
#ifndef AUM_EMU
template <class T, int PHASE, int SP, bool HAS_Z>
__global__ __launch_bounds__(SCANT_NW * 64, AUM_SCANT_BWD_MINW) void k_scant_seg_bwd(AumScanTmBwdArgs a, ScanTBwdOut wo, ScanTSeg sg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanTBwdLds<T>::n];
    scant_seg_bwd<T, PHASE, SP, HAS_Z>(a, wo, sg, (int)blockIdx.x, lds);
}
#endif
template <class T, int PHASE, int SP, bool HAS_Z>
static int launch_scant_seg_bwd(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, aum_stream_t s) {
    const int grid = (a.batch * (a.dim / WAVE) * sg.nseg + SCANT_NW - 1) / SCANT_NW;
    return AUM_LAUNCH(grid, SCANT_NW * 64, s, (ScanTBwdLds<T>{}), (k_scant_seg_bwd<T, PHASE, SP, HAS_Z>), (scant_seg_bwd<T, PHASE, SP, HAS_Z>(a, wo, sg, wg, lds)), a, wo, sg);
}
template <class T> static int scan_tm_seg_bwd_t(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s) {
    if (a.flags & AUM_SCAN_DELTA_ACTIVATED) {
        if constexpr (sizeof(T) == 2) return with_int<0, 1, 2>(phase, [&](auto ph) { return launch_scant_seg_bwd<T, ph, SCANT_SP_ACT, true>(a, wo, sg, s); });
        return AUM_E_UNSUPPORTED;
    }
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) { return with_bool(a.z != nullptr, [&](auto hz) {
        return with_int<0, 1, 2>(phase, [&](auto ph) { return launch_scant_seg_bwd<T, ph, sp ? SCANT_SP_IN : SCANT_SP_NONE, hz>(a, wo, sg, s); }); }); });
}
#if AUM_HAS_DTYPE(0)
int scan_tm_bwd_f32(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s) { return scan_tm_bwd_t<float>(a, wo, s); }
int scan_tm_seg_bwd_f32(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_bwd_t<float>(a, wo, sg, phase, s); }
#endif
#if AUM_HAS_DTYPE(1)
int scan_tm_bwd_bf16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s) { return scan_tm_bwd_t<bf16_t>(a, wo, s); }
int scan_tm_seg_bwd_bf16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_bwd_t<bf16_t>(a, wo, sg, phase, s); }
#endif
#if AUM_HAS_DTYPE(2)
int scan_tm_bwd_f16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, aum_stream_t s) { return scan_tm_bwd_t<f16_t>(a, wo, s); }
int scan_tm_seg_bwd_f16(const AumScanTmBwdArgs& a, const ScanTBwdOut& wo, const ScanTSeg& sg, int phase, aum_stream_t s) { return scan_tm_seg_bwd_t<f16_t>(a, wo, sg, phase, s); }
#endif
#endif

}  // namespace aum

#if AUM_API_PART == 3 || AUM_API_PART == 0
AUM_API int32_t aum_scan_tm_nck(int32_t len) { return len > 0 ? scant_nck(len) : 0; }
AUM_API int32_t aum_scan_tm_ckpt_rows(int32_t dtype) {
    return dtype == AUM_F32 ? scant_ck_rows<float>() : (dtype == AUM_BF16 || dtype == AUM_F16) ? scant_ck_rows<bf16_t>() : 0;
}

// AUM_SCAN_DELTA_ACTIVATED (16-bit activations with z): delta already holds softplus(raw + delta_bias).  The forward reads it as it is -- the
// kernels without bias and softplus; the backward keeps the softplus derivative (SCANT_SP_ACT) and still writes ddelta_bias.
static bool scan_tm_act_ok(uint32_t flags, int32_t dtype, const void* z) { return !(flags & AUM_SCAN_DELTA_ACTIVATED) || (dtype != AUM_F32 && z); }
template <class A> static A scan_tm_fwd_resolve(const A& a) {       // the kernels' view of a forward's arguments (fixed batch, chunk, packed chunk)
    A r = a;
    if (a.flags & AUM_SCAN_DELTA_ACTIVATED) {
        r.delta_bias = nullptr;
        r.flags &= ~(AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED);
    }
    return r;
}
static int scan_tm_fwd_check(const AumScanTmFwdArgs* a) {
    if (!a) return AUM_E_NULL;
    if (!a->u || !a->delta || !a->B || !a->C || !a->A || !a->out) return AUM_E_NULL;
    if (a->batch <= 0 || a->dim <= 0 || a->len <= 0 || a->dstate <= 0) return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2) return AUM_E_DTYPE;
    if (!scant_supported(a->dim, a->dstate)) return AUM_E_UNSUPPORTED;
    if (!scan_tm_act_ok(a->flags, a->dtype, a->z)) return AUM_E_UNSUPPORTED;
    if (a->A_b && (a->flags & AUM_SCAN_REVERSE)) return AUM_E_UNSUPPORTED;
    if (a->dtype != AUM_F32) {      // 16-bit B / C rows are read as dwords through the scalar cache
        if ((a->B_bs | a->B_ts | a->C_bs | a->C_ts) & 1) return AUM_E_UNSUPPORTED;
        if ((((uintptr_t)a->B) | ((uintptr_t)a->C)) & 3) return AUM_E_UNSUPPORTED;
    }
    {       // row offsets inside a batch entry are 32-bit byte cursors
        const int64_t es = a->dtype == AUM_F32 ? 4 : 2, lim = ((int64_t)1 << 31) - 1;
        const int64_t ts[] = {a->u_ts, a->delta_ts, a->z ? a->z_ts : 0, a->out_ts, a->out_pre ? a->pre_ts : 0, a->B_ts, a->C_ts};
        for (int64_t t : ts)
            if (t < 0 || t * es * a->len > lim) return AUM_E_UNSUPPORTED;
        if ((int64_t)scant_nck(a->len) * a->dstate * a->dim * 4 > lim) return AUM_E_UNSUPPORTED;
        // rows are moved as 16-byte chunks
        const uintptr_t ptrs = (uintptr_t)a->u | (uintptr_t)a->delta | (uintptr_t)a->z | (uintptr_t)a->out | (uintptr_t)a->out_pre;
        const int64_t strides = a->u_bs | a->u_ts | a->delta_bs | a->delta_ts | (a->z ? (a->z_bs | a->z_ts) : 0) | a->out_bs | a->out_ts |
                                (a->out_pre ? (a->pre_bs | a->pre_ts) : 0);
        if ((ptrs & 15) || ((strides * es) & 15)) return AUM_E_UNSUPPORTED;
    }
    return AUM_OK;
}
AUM_API int aum_scan_tm_fwd(const AumScanTmFwdArgs* a, void* stream) {
    const int rc = scan_tm_fwd_check(a);
    if (rc != AUM_OK) return rc;
    aum_stream_t s = (aum_stream_t)stream;
    const AumScanTmFwdArgs k = scan_tm_fwd_resolve(*a);
    return AUM_BY_DTYPE_X(k.dtype, scan_tm_fwd, k, s);
}
static int scan_tm_seg_fwd_any(const AumScanTmFwdArgs& a, const ScanTSeg& sg, int phase, aum_stream_t s) {
    return AUM_BY_DTYPE_X(a.dtype, scan_tm_seg_fwd, a, sg, phase, s);
}
AUM_API int64_t aum_scan_tm_seg_carry_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional, int32_t segments) {
    if (batch <= 0 || dim <= 0 || len <= 0 || segments < 2 || !scant_supported(dim, dstate)) return 0;
    return scant_seg_carry_floats(batch, dim, segments, bidirectional != 0) * (int64_t)sizeof(float);
}
AUM_API int aum_scan_tm_seg_fwd(const AumScanTmSegFwdArgs* sa, void* stream) {
    if (!sa) return AUM_E_NULL;
    const AumScanTmFwdArgs* a = &sa->base;
    const int rc = scan_tm_fwd_check(a);
    if (rc != AUM_OK) return rc;
    if (sa->segments < 2 || sa->segments > AUM_SCAN_TM_MAX_SEGMENTS) return AUM_E_SHAPE;
    if (!sa->carry) return AUM_E_NULL;
    const bool bidir = a->A_b != nullptr;
    if (sa->carry_bytes < scant_seg_carry_floats(a->batch, a->dim, sa->segments, bidir) * (int64_t)sizeof(float)) return AUM_E_WORKSPACE;
    aum_stream_t s = (aum_stream_t)stream;
    ScanTSeg sg;
    sg.carry = sa->carry;
    sg.nseg = sa->segments;
    sg.seg_len = scant_seg_len(a->len, sa->segments);
    sg.dir0 = 0;
    sg.ndl = bidir ? 2 : 1;
    const AumScanTmFwdArgs k = scan_tm_fwd_resolve(*a);
    int r = scan_tm_seg_fwd_any(k, sg, 3, s);
    if (r != AUM_OK) return r;
    sg.ndl = 1;
    if (!bidir) return scan_tm_seg_fwd_any(k, sg, 0, s);
    r = scan_tm_seg_fwd_any(k, sg, 1, s);
    if (r != AUM_OK) return r;
    sg.dir0 = 1;
    return scan_tm_seg_fwd_any(k, sg, 2, s);
}
AUM_API int aum_scan_tm_fwd_state(const AumScanTmFwdStateArgs* sa, void* stream) {
    if (!sa) return AUM_E_NULL;
    const AumScanTmFwdArgs* a = &sa->base;
    const int rc = scan_tm_fwd_check(a);
    if (rc != AUM_OK) return rc;
    // an inference path: one direction, forward time, no checkpoints, no pre-gate copy
    if (a->A_b || a->ckpt || a->out_pre || (a->flags & AUM_SCAN_REVERSE)) return AUM_E_UNSUPPORTED;
    if ((((uintptr_t)sa->state_in) | ((uintptr_t)sa->state_out)) & 15) return AUM_E_UNSUPPORTED;      // 16-byte accesses
    if ((int64_t)a->dim * a->dstate * 4 > (((int64_t)1 << 31) - 1)) return AUM_E_UNSUPPORTED;              // 32-bit byte offsets inside a state row
    if (sa->segments < 1 || sa->segments > AUM_SCAN_TM_MAX_SEGMENTS) return AUM_E_SHAPE;
    aum_stream_t s = (aum_stream_t)stream;
    const AumScanTmFwdArgs k = scan_tm_fwd_resolve(*a);
    const ScanTState st = {sa->state_in, sa->state_out};
    auto run = [&](const ScanTSeg* sg, int phase) {
        return AUM_BY_DTYPE_X(k.dtype, scan_tm_fwd_state, k, st, sg, phase, s);
    };
    if (sa->segments == 1) return run(nullptr, 0);
    if (!sa->carry) return AUM_E_NULL;
    if (sa->carry_bytes < scant_seg_carry_floats(a->batch, a->dim, sa->segments, false) * (int64_t)sizeof(float)) return AUM_E_WORKSPACE;
    ScanTSeg sg;
    sg.carry = sa->carry;
    sg.nseg = sa->segments;
    sg.seg_len = scant_seg_len(a->len, sa->segments);
    sg.dir0 = 0;
    sg.ndl = 1;
    const int r = run(&sg, 3);
    if (r != AUM_OK) return r;
    return run(&sg, 0);
}
AUM_API int64_t aum_scan_tm_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional) {
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0 || !scant_supported(dim, dstate)) return 0;
    return scant_ws_layout(batch, dim, len, dstate, bidirectional != 0).total * (int64_t)sizeof(float);
}

// sums of the backward's partials: dBC[b][t][k] over the channel-group partials, dA[e][n] over (batch entry) per direction,
// dD[e] / ddelta_bias[e] over (direction, batch entry)
struct ScanTReduceArgs {
    const float* ws;
    float *dBC, *dA, *dA_b, *dD, *dbias;
    const float *A, *A_b;           // with dAx / dAx_b: the products dA .* A, dA_b .* A_b are written next to dA / dA_b
    float *dAx, *dAx_b;
    int64_t o_dA, o_dD, o_dbias;
    int32_t batch, pbatch, dim, len, dstate, nparts, ndir;       // pbatch: rows of dA / dD / ddelta_bias partials per direction
    int32_t nsum;                                                // partial dB | dC rows of a token to add: the first nsum of its nparts slots
};
#ifndef AUM_EMU
__global__ __launch_bounds__(256) void k_scant_bwd_reduce(ScanTReduceArgs a) {
    const int64_t ntok = (int64_t)a.batch * a.len;
    const int k4 = 2 * a.dstate / 4;                                  // float4 columns of a dB | dC row
    const int64_t n_bc = ntok * k4;
    const int64_t n_a = (int64_t)a.ndir * a.dim * a.dstate;
    const int64_t n_d = 2 * (int64_t)a.dim;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_bc + n_a + n_d; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n_bc) {
            const int64_t tok = i / k4;
            const int c = (int)(i % k4);
            const float4* src = reinterpret_cast<const float4*>(a.ws) + (tok * a.nparts) * k4 + c;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
            for (int q = 0; q < a.nsum; ++q) {
                const float4 v = src[(int64_t)q * k4];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            reinterpret_cast<float4*>(a.dBC)[i] = acc;
        } else if (i < n_bc + n_a) {
            const int64_t r = i - n_bc;
            const int d = (int)(r / ((int64_t)a.dim * a.dstate));
            const int64_t en = r % ((int64_t)a.dim * a.dstate);
            const int e = (int)(en / a.dstate), n = (int)(en % a.dstate);
            const float* src = a.ws + a.o_dA + (int64_t)d * a.pbatch * a.dstate * a.dim + (int64_t)n * a.dim + e;
            // (unrolled: the loads of a group are in flight together -- rolled, every one of the 64 was a round trip to memory on the
            // critical path of the kernel; the order of the additions is unchanged)
            float acc = 0.f;
#pragma unroll 16
            for (int b = 0; b < a.pbatch; ++b) acc += src[(int64_t)b * a.dstate * a.dim];
            (d ? a.dA_b : a.dA)[en] = acc;
            float* px = d ? a.dAx_b : a.dAx;
            if (px) px[en] = acc * (d ? a.A_b : a.A)[en];
        } else {
            const int64_t r = i - n_bc - n_a;
            const bool is_bias = r >= a.dim;
            const int e = (int)(r % a.dim);
            float* dst = is_bias ? a.dbias : a.dD;
            if (!dst) continue;
            const float* src = a.ws + (is_bias ? a.o_dbias : a.o_dD) + e;
            float acc = 0.f;
#pragma unroll 16
            for (int q = 0; q < a.ndir * a.pbatch; ++q) acc += src[(int64_t)q * a.dim];
            dst[e] = acc;
        }
    }
}
#endif
#ifdef AUM_EMU
static void scant_reduce_host(const ScanTReduceArgs& a) {      // what k_scant_bwd_reduce computes, as plain loops
    const int64_t ntok = (int64_t)a.batch * a.len;
    const int K = 2 * a.dstate;
    for (int64_t tok = 0; tok < ntok; ++tok)
        for (int k = 0; k < K; ++k) {
            float acc = 0.f;
            for (int q = 0; q < a.nsum; ++q) acc += a.ws[(tok * a.nparts + q) * K + k];
            a.dBC[tok * K + k] = acc;
        }
    for (int d = 0; d < a.ndir; ++d)
        for (int e = 0; e < a.dim; ++e)
            for (int n = 0; n < a.dstate; ++n) {
                float acc = 0.f;
                for (int b = 0; b < a.pbatch; ++b) acc += a.ws[a.o_dA + (((int64_t)d * a.pbatch + b) * a.dstate + n) * a.dim + e];
                (d ? a.dA_b : a.dA)[(int64_t)e * a.dstate + n] = acc;
                float* px = d ? a.dAx_b : a.dAx;
                if (px) px[(int64_t)e * a.dstate + n] = acc * (d ? a.A_b : a.A)[(int64_t)e * a.dstate + n];
            }
    for (int e = 0; e < a.dim; ++e) {
        float accD = 0.f, accb = 0.f;
        for (int q = 0; q < a.ndir * a.pbatch; ++q) {
            accD += a.ws[a.o_dD + (int64_t)q * a.dim + e];
            accb += a.ws[a.o_dbias + (int64_t)q * a.dim + e];
        }
        if (a.dD) a.dD[e] = accD;
        if (a.dbias) a.dbias[e] = accb;
    }
}
#endif
static int scant_reduce_launch(const ScanTReduceArgs& a, aum_stream_t s) {
    return AUM_LAUNCH(2048, 256, s, (NoLds{}), k_scant_bwd_reduce, (AUM_HOST_LOOP(scant_reduce_host(a))), a);
}

static int scan_tm_bwd_any(const AumScanTmBwdArgs* a, int nseg, void* stream) {
    if (!a) return AUM_E_NULL;
    if (!a->u || !a->delta || !a->B || !a->C || !a->A || !a->dout || !a->ckpt) return AUM_E_NULL;
    if (!a->du || !a->ddelta || !a->dA || !a->dBC || !a->workspace) return AUM_E_NULL;
    if (a->z && (!a->out_pre || !a->dz)) return AUM_E_NULL;
    if (a->A_b && !a->dA_b) return AUM_E_NULL;
    if (a->batch <= 0 || a->dim <= 0 || a->len <= 0 || a->dstate <= 0) return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2) return AUM_E_DTYPE;
    if (!scant_supported(a->dim, a->dstate)) return AUM_E_UNSUPPORTED;
    if (a->A_b && (a->flags & AUM_SCAN_REVERSE)) return AUM_E_UNSUPPORTED;
    if (!scan_tm_act_ok(a->flags, a->dtype, a->z)) return AUM_E_UNSUPPORTED;
    const int64_t es = a->dtype == AUM_F32 ? 4 : 2, lim = ((int64_t)1 << 31) - 1;
    if (a->dtype != AUM_F32) {
        if ((a->B_bs | a->B_ts | a->C_bs | a->C_ts) & 1) return AUM_E_UNSUPPORTED;
        if ((((uintptr_t)a->B) | ((uintptr_t)a->C)) & 3) return AUM_E_UNSUPPORTED;
    }
    {
        const int64_t ts[] = {a->u_ts, a->delta_ts, a->z ? a->z_ts : 0, a->dout_ts, a->z ? a->pre_ts : 0, a->du_ts, a->ddelta_ts, a->z ? a->dz_ts : 0,
                              a->B_ts, a->C_ts};
        for (int64_t t : ts)
            if (t < 0 || t * es * a->len > lim) return AUM_E_UNSUPPORTED;
        const uintptr_t ptrs = (uintptr_t)a->u | (uintptr_t)a->delta | (uintptr_t)a->z | (uintptr_t)a->dout | (uintptr_t)a->out_pre | (uintptr_t)a->du |
                               (uintptr_t)a->ddelta | (uintptr_t)a->dz;
        const int64_t strides = a->u_bs | a->u_ts | a->delta_bs | a->delta_ts | a->dout_bs | a->dout_ts | a->du_bs | a->du_ts | a->ddelta_bs | a->ddelta_ts |
                                (a->z ? (a->z_bs | a->z_ts | a->pre_bs | a->pre_ts | a->dz_bs | a->dz_ts) : 0);
        if ((ptrs & 15) || ((strides * es) & 15)) return AUM_E_UNSUPPORTED;
    }
    const bool bidir = a->A_b != nullptr;
    if (nseg != 1 && (nseg < 2 || nseg > AUM_SCAN_TM_MAX_SEGMENTS)) return AUM_E_SHAPE;
    const ScanTWs L = scant_ws_layout(a->batch, a->dim, a->len, a->dstate, bidir, nseg);
    if (a->workspace_bytes < L.total * (int64_t)sizeof(float)) return AUM_E_WORKSPACE;
    if ((int64_t)a->len * L.nparts * 2 * a->dstate * 4 > lim || (int64_t)scant_nck(a->len) * a->dstate * a->dim * 4 > lim) return AUM_E_UNSUPPORTED;
    float* ws = (float*)a->workspace;
    ScanTBwdOut wo;
    wo.dbc = ws + L.dbc;
    wo.dA = ws + L.dA;
    wo.dD = ws + L.dD;
    wo.dbias = ws + L.dbias;
    wo.nparts = L.nparts;
    wo.carry = ws + L.carry;
    wo.trace = nullptr;
#ifdef AUM_SCANT_TRACE
    wo.trace = reinterpret_cast<unsigned long long*>(ws + L.trace);
#endif
    aum_stream_t s = (aum_stream_t)stream;
    const bool act = (a->flags & AUM_SCAN_DELTA_ACTIVATED) != 0;
    AumScanTmBwdArgs k = *a;            // the kernels' view: an activated delta carries its bias already
    if (act) k.delta_bias = nullptr;
    int rc = AUM_OK;
    if (nseg == 1) {
        rc = AUM_BY_DTYPE_X(k.dtype, scan_tm_bwd, k, wo, s);
    } else {
        ScanTSeg sg;
        sg.carry = ws + L.carry;
        sg.nseg = nseg;
        sg.seg_len = scant_seg_len(a->len, nseg);
        sg.dir0 = 0;
        sg.ndl = bidir ? 2 : 1;
        {       // adjoint carries: the forward's run function on (dout, delta, z, C) with the time mapping reversed (PHASE 4)
            AumScanTmFwdArgs f = {};
            f.u = a->dout; f.u_bs = a->dout_bs; f.u_ts = a->dout_ts;
            f.delta = a->delta; f.delta_bs = a->delta_bs; f.delta_ts = a->delta_ts;
            f.z = a->z; f.z_bs = a->z_bs; f.z_ts = a->z_ts;
            f.B = a->C; f.B_bs = a->C_bs; f.B_ts = a->C_ts;
            f.C = a->C; f.C_bs = a->C_bs; f.C_ts = a->C_ts;
            f.A = a->A; f.A_b = a->A_b; f.delta_bias = a->delta_bias;
            f.out = a->du; f.out_bs = a->du_bs; f.out_ts = a->du_ts;       // never written by a carry pass
            f.batch = a->batch; f.dim = a->dim; f.len = a->len; f.dstate = a->dstate; f.dtype = a->dtype; f.flags = a->flags;
            rc = scan_tm_seg_fwd_any(scan_tm_fwd_resolve(f), sg, 4, s);
            if (rc != AUM_OK) return rc;
        }
        sg.ndl = 1;
        for (int d = 0; d < (bidir ? 2 : 1) && rc == AUM_OK; ++d) {
            sg.dir0 = d;
            const int phase = bidir ? 1 + d : 0;
            rc = AUM_BY_DTYPE_X(k.dtype, scan_tm_seg_bwd, k, wo, sg, phase, s);
        }
    }
    if (rc != AUM_OK) return rc;
    ScanTReduceArgs r;
    r.ws = ws;
    r.dBC = a->dBC; r.dA = a->dA; r.dA_b = a->dA_b; r.dD = a->D ? a->dD : nullptr; r.dbias = a->delta_bias || act ? a->ddelta_bias : nullptr;
    r.o_dA = L.dA; r.o_dD = L.dD; r.o_dbias = L.dbias;
    r.A = a->A; r.A_b = a->A_b; r.dAx = a->dA_xA; r.dAx_b = a->A_b ? a->dA_b_xA : nullptr;
    r.batch = a->batch; r.pbatch = a->batch * nseg; r.dim = a->dim; r.len = a->len; r.dstate = a->dstate; r.nparts = L.nparts; r.ndir = L.ndir; r.nsum = scant_dbc_rows_to_sum(L.nparts, bidir);
    return scant_reduce_launch(r, s);
}
AUM_API int aum_scan_tm_bwd(const AumScanTmBwdArgs* a, void* stream) { return scan_tm_bwd_any(a, 1, stream); }
AUM_API int aum_scan_tm_seg_bwd(const AumScanTmSegBwdArgs* sa, void* stream) {
    if (!sa) return AUM_E_NULL;
    if (sa->segments < 2) return AUM_E_SHAPE;
    return scan_tm_bwd_any(&sa->base, sa->segments, stream);
}
AUM_API int64_t aum_scan_tm_seg_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional, int32_t segments) {
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0 || segments < 2 || segments > AUM_SCAN_TM_MAX_SEGMENTS || !scant_supported(dim, dstate)) return 0;
    return scant_ws_layout(batch, dim, len, dstate, bidirectional != 0, segments).total * (int64_t)sizeof(float);
}
// ---- token-major causal conv1d ------------------------------------------------------------------
#ifndef AUM_EMU
template <class T, bool SILU> AUM_GLOBAL void k_convt_fwd(AumConvTmArgs a) { convt_fwd_wave<T, SILU>(a, (int)blockIdx.x); }
template <class T, bool SILU> AUM_GLOBAL void k_convt_bwd(AumConvTmArgs a) { convt_bwd_wave<T, SILU>(a, (int)blockIdx.x); }
#endif
template <class T, bool SILU> static int convt_launch(const AumConvTmArgs& a, bool bwd, aum_stream_t s) {
    const int grid = bwd ? a.batch * convt_chunks<true>(a.len) * convt_cblocks<T, true>(a.dim) : a.batch * convt_chunks<false>(a.len) * convt_cblocks<T, false>(a.dim);
    if (bwd) return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_bwd<T, SILU>), (convt_bwd_wave<T, SILU>(a, wg)), a);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_fwd<T, SILU>), (convt_fwd_wave<T, SILU>(a, wg)), a);
}
template <class T> static int convt_dispatch_t(const AumConvTmArgs& a, bool bwd, aum_stream_t s) {
    return with_bool((a.flags & AUM_CONV_SILU) != 0, [&](auto silu) { return convt_launch<T, silu>(a, bwd, s); });
}
static int convt_dispatch(const AumConvTmArgs* a, bool bwd, void* stream) {
    if (!a || !a->x || !a->weight) return AUM_E_NULL;
    if (bwd ? (!a->dy || !a->dx || !a->dw_part) : !a->y) return AUM_E_NULL;
    if (bwd && a->bias && !a->db_part) return AUM_E_NULL;
    if (a->batch <= 0 || a->dim <= 0 || a->len <= 0 || a->width <= 0) return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2) return AUM_E_DTYPE;
    if (a->width > CONVT_W) return AUM_E_UNSUPPORTED;
    const int64_t es = a->dtype == AUM_F32 ? 4 : 2;
    if (a->dim % (16 / es)) return AUM_E_UNSUPPORTED;
    const uintptr_t ptrs = (uintptr_t)a->x | (uintptr_t)(bwd ? a->dy : a->y) | (uintptr_t)(bwd ? a->dx : a->y) | (uintptr_t)a->weight |
                           (uintptr_t)a->bias;
    const int64_t strides = a->x_bs | a->x_ts | (bwd ? (a->dy_bs | a->dy_ts | a->dx_bs | a->dx_ts) : (a->y_bs | a->y_ts));
    if ((ptrs & 15) || ((strides * es) & 15)) return AUM_E_UNSUPPORTED;
    const int64_t lim = (int64_t)1 << 31;       // buffer offsets are 32-bit: one batch entry's rows must fit
    const int64_t ts = a->x_ts > (bwd ? (a->dy_ts > a->dx_ts ? a->dy_ts : a->dx_ts) : a->y_ts) ? a->x_ts : (bwd ? (a->dy_ts > a->dx_ts ? a->dy_ts : a->dx_ts) : a->y_ts);
    if ((int64_t)a->len * ts * es >= lim) return AUM_E_UNSUPPORTED;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a->dtype, convt_dispatch_t, *a, bwd, s);
}
AUM_API int aum_conv1d_tm_fwd(const AumConvTmArgs* a, void* stream) { return convt_dispatch(a, false, stream); }
AUM_API int aum_conv1d_tm_bwd(const AumConvTmArgs* a, void* stream) { return convt_dispatch(a, true, stream); }
/* 1 when this build sums the dB / dC terms of 16-bit activations on the matrix pipe (terms rounded to bf16): tests bound them accordingly */
AUM_API int32_t aum_conv1d_tm_nparts(int32_t batch, int32_t len) { return batch > 0 && len > 0 ? convt_nparts(batch, len) : 0; }

// ---- operand checks of the streaming entry points: what the three conv entries share, and what the three scan entries share ----
// Each entry hands in what differs: `var` (packed sessions, else nullptr), counts_ok (its own row counts > 0), rows (the most rows a 32-bit
// byte cursor spans: len or total), allowed (flag bits it takes), fits (its own limits), units (grid factor next to the channel blocks; 0: none).
// Refusals in this order: AUM_E_NULL (operands), the packed map's code, AUM_E_SHAPE, AUM_E_DTYPE, then AUM_E_UNSUPPORTED for everything else.
struct StreamVar { const int32_t *cu_seqlens, *state_indices; int total, nseq, nrows; };
static int stream_var_check(const StreamVar* v) {
    if (!v) return AUM_OK;
    if (!v->cu_seqlens) return AUM_E_NULL;
    if (v->total <= 0 || v->nseq <= 0 || v->nrows <= 0) return AUM_E_SHAPE;
    if (((uintptr_t)v->cu_seqlens | (uintptr_t)v->state_indices) & 3) return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
// bs: x_bs | y_bs where batch strides exist, else 0
template <class A> static int conv_stream_check(const A& a, const StreamVar* var, bool counts_ok, int64_t rows, int64_t bs, uint32_t allowed, bool fits,
                                                int64_t units) {
    if (!a.x || !a.conv_state || !a.weight || !a.y) return AUM_E_NULL;
    if (const int rc = stream_var_check(var)) return rc;
    if (a.dim <= 0 || a.width <= 0 || !counts_ok) return AUM_E_SHAPE;
    if (a.dtype < 0 || a.dtype > 2) return AUM_E_DTYPE;
    if (a.width > CONVT_W || !fits || (a.flags & ~allowed)) return AUM_E_UNSUPPORTED;
    const int64_t es = a.dtype == AUM_F32 ? 4 : 2;
    if (a.dim % (16 / es)) return AUM_E_UNSUPPORTED;
    if (a.x_ts < 0 || a.y_ts < 0) return AUM_E_UNSUPPORTED;
    const uintptr_t ptrs = (uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.weight | (uintptr_t)a.bias;
    if ((ptrs & 15) || (((bs | a.x_ts | a.y_ts) * es) & 15) || ((uintptr_t)a.conv_state & 3)) return AUM_E_UNSUPPORTED;
    if (a.x == a.y) return AUM_E_UNSUPPORTED;      // rows are fetched ahead of the steps that write them
    const int64_t lim = (int64_t)1 << 31;         // buffer offsets are 32-bit: the rows of one batch entry / one sequence must fit
    if (rows * (a.x_ts > a.y_ts ? a.x_ts : a.y_ts) * es >= lim || (int64_t)a.dim * a.width * 4 >= lim) return AUM_E_UNSUPPORTED;
    if (units * convt_cblocks<float, false>(a.dim) >= lim) return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
// rows16: the rows move as 16-byte chunks and B / C as dwords (the state in / state out kernels); else element by element (the chunk kernels)
template <class A> static int scan_stream_check(const A& a, const StreamVar* var, bool counts_ok, int64_t rows, uint32_t allowed, bool fits, int64_t units,
                                                bool rows16) {
    if (!a.u || !a.delta || !a.B || !a.C || !a.A || !a.state || !a.out) return AUM_E_NULL;
    if (const int rc = stream_var_check(var)) return rc;
    if (a.dim <= 0 || a.dstate <= 0 || !counts_ok) return AUM_E_SHAPE;
    if (a.dtype < 0 || a.dtype > 2) return AUM_E_DTYPE;
    if (!scant_supported(a.dim, a.dstate) || !fits || (a.flags & ~allowed)) return AUM_E_UNSUPPORTED;
    if (rows16 && !scan_tm_act_ok(a.flags, a.dtype, a.z)) return AUM_E_UNSUPPORTED;
    const int64_t es = a.dtype == AUM_F32 ? 4 : 2, lim = ((int64_t)1 << 31) - 1;
    if (rows16 && a.dtype != AUM_F32 && (((a.B_ts | a.C_ts) & 1) || ((((uintptr_t)a.B) | ((uintptr_t)a.C)) & 3))) return AUM_E_UNSUPPORTED;
    const int64_t ts[] = {a.u_ts, a.delta_ts, a.z ? a.z_ts : 0, a.out_ts, a.B_ts, a.C_ts};      // row offsets are 32-bit byte cursors
    for (int64_t t : ts)
        if (t < 0 || (t + a.dim) * es * rows > lim) return AUM_E_UNSUPPORTED;
    if ((int64_t)a.dim * a.dstate * 4 > lim || units * (a.dim / WAVE) > lim) return AUM_E_UNSUPPORTED;
    const uintptr_t rowp = (uintptr_t)a.u | (uintptr_t)a.delta | (uintptr_t)a.z | (uintptr_t)a.out;
    if (rows16) {
        const int64_t strides = a.u_ts | a.delta_ts | (a.z ? a.z_ts : 0) | a.out_ts;
        if (((rowp | (uintptr_t)a.state) & 15) || ((strides * es) & 15)) return AUM_E_UNSUPPORTED;
    } else if (((rowp | (uintptr_t)a.B | (uintptr_t)a.C) & (uintptr_t)(es - 1)) || ((uintptr_t)a.state & 15)) {
        return AUM_E_UNSUPPORTED;       // elements aligned; a channel's states move as 16-byte chunks
    }
    return AUM_OK;
}

// ---- chunked streaming inference (stream_tm_kernels.h): T tokens per call from carried caches ------
#ifndef AUM_EMU
template <class T, bool SILU> AUM_GLOBAL void k_convt_chunk(AumConvTmChunkArgs a) { convc_wave<T, SILU>(a, (int)blockIdx.x); }
template <class T, bool SP, bool HAS_Z> AUM_GLOBAL void k_stream_scan_chunk(AumScanTmChunkArgs a) { scanc_wave<T, SP, HAS_Z>(a, (int)blockIdx.x); }
template <class T, bool SILU, bool PEEK = false> AUM_GLOBAL void k_convt_chunk_var(AumConvTmChunkVarArgs a) { convc_var_wave<T, SILU, PEEK>(a, (int)blockIdx.x); }
template <class T, bool SP, bool HAS_Z, bool PEEK = false> AUM_GLOBAL void k_stream_scan_chunk_var(AumScanTmChunkVarArgs a) {
    scanc_var_wave<T, SP, HAS_Z, PEEK>(a, (int)blockIdx.x);
}
template <class T, bool SILU> AUM_GLOBAL void k_convt_chunk_peeks(AumConvTmChunkVarArgs a, int pe) { convc_var_wave<T, SILU, false, true>(a, (int)blockIdx.x, pe); }
template <class T, bool SP, bool HAS_Z> AUM_GLOBAL void k_stream_scan_chunk_peeks(AumScanTmChunkVarArgs a, int pe) {
    scanc_var_wave<T, SP, HAS_Z, false, true>(a, (int)blockIdx.x, pe);
}
#endif
template <class T, bool SILU> static int convc_launch(const AumConvTmChunkArgs& a, aum_stream_t s) {
    const int grid = a.batch * convt_cblocks<T, false>(a.dim);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_chunk<T, SILU>), (convc_wave<T, SILU>(a, wg)), a);
}
template <class T> static int convc_dispatch_t(const AumConvTmChunkArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_CONV_SILU) != 0, [&](auto silu) { return convc_launch<T, silu>(a, s); });
}
AUM_API int aum_conv1d_tm_chunk(const AumConvTmChunkArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    if (const int rc = conv_stream_check(*a, nullptr, a->batch > 0 && a->len > 0, a->len, a->x_bs | a->y_bs, ~(uint32_t)AUM_CONV_PEEK_LAST, true, 0)) return rc;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a->dtype, convc_dispatch_t, *a, s);
}
template <class T, bool SP, bool HAS_Z> static int scanc_launch(const AumScanTmChunkArgs& a, aum_stream_t s) {
    const int grid = a.batch * (a.dim / WAVE);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_stream_scan_chunk<T, SP, HAS_Z>), (scanc_wave<T, SP, HAS_Z>(a, wg)), a);
}
template <class T> static int scanc_dispatch_t(const AumScanTmChunkArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) { return with_bool(a.z != nullptr, [&](auto hz) { return scanc_launch<T, sp, hz>(a, s); }); });
}
AUM_API int aum_scan_tm_chunk(const AumScanTmChunkArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    if (const int rc = scan_stream_check(*a, nullptr, a->batch > 0 && a->len > 0, a->len, AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED, true, 0, false)) return rc;
    const AumScanTmChunkArgs k = scan_tm_fwd_resolve(*a);
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(k.dtype, scanc_dispatch_t, k, s);
}

// ---- the same on packed sessions: (sequence, channel block) units, rows and cache row from cu_seqlens / state_indices ----
template <class T, bool SILU, bool PEEK> static int convcv_launch(const AumConvTmChunkVarArgs& a, aum_stream_t s) {
    const int grid = a.nseq * convt_cblocks<T, false>(a.dim);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_chunk_var<T, SILU, PEEK>), (convc_var_wave<T, SILU, PEEK>(a, wg)), a);
}
template <class T> static int convcv_dispatch_t(const AumConvTmChunkVarArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_CONV_PEEK_LAST) != 0, [&](auto peek) { return with_bool((a.flags & AUM_CONV_SILU) != 0, [&](auto silu) { return convcv_launch<T, silu, peek>(a, s); }); });
}
AUM_API int aum_conv1d_tm_chunk_var(const AumConvTmChunkVarArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = conv_stream_check(*a, &var, true, a->total, 0, ~0u, true, a->nseq)) return rc;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a->dtype, convcv_dispatch_t, *a, s);
}
template <class T, bool SP, bool HAS_Z, bool PEEK> static int scancv_launch(const AumScanTmChunkVarArgs& a, aum_stream_t s) {
    const int grid = a.nseq * (a.dim / WAVE);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_stream_scan_chunk_var<T, SP, HAS_Z, PEEK>), (scanc_var_wave<T, SP, HAS_Z, PEEK>(a, wg)), a);
}
template <class T> static int scancv_dispatch_t(const AumScanTmChunkVarArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_SCAN_PEEK_LAST) != 0, [&](auto peek) { return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        return with_bool(a.z != nullptr, [&](auto hz) { return scancv_launch<T, sp, hz, peek>(a, s); }); }); });
}
AUM_API int aum_scan_tm_chunk_var(const AumScanTmChunkVarArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = scan_stream_check(*a, &var, true, a->total, AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED | AUM_SCAN_PEEK_LAST, true, a->nseq, false)) return rc;
    const AumScanTmChunkVarArgs k = scan_tm_fwd_resolve(*a);
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(k.dtype, scancv_dispatch_t, k, s);
}

// ---- packed sessions with a peek row behind every peek_every rows (PEEKS of convc_unit / scanc_unit): the operands, checks and grids of
// the packed entry points above; the PEEK_LAST flags are not theirs (AUM_E_UNSUPPORTED), peek_every < 1 is AUM_E_SHAPE ----
template <class T, bool SILU> static int convcp_launch(const AumConvTmChunkVarArgs& a, int pe, aum_stream_t s) {
    const int grid = a.nseq * convt_cblocks<T, false>(a.dim);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_chunk_peeks<T, SILU>), (convc_var_wave<T, SILU, false, true>(a, wg, pe)), a, pe);
}
template <class T> static int convcp_dispatch_t(const AumConvTmChunkVarArgs& a, int pe, aum_stream_t s) {
    return with_bool((a.flags & AUM_CONV_SILU) != 0, [&](auto silu) { return convcp_launch<T, silu>(a, pe, s); });
}
AUM_API int aum_conv1d_tm_chunk_peeks(const AumConvTmChunkPeeksArgs* pa, void* stream) {
    if (!pa) return AUM_E_NULL;
    const AumConvTmChunkVarArgs* a = &pa->base;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = conv_stream_check(*a, &var, pa->peek_every >= 1, a->total, 0, ~(uint32_t)AUM_CONV_PEEK_LAST, true, a->nseq)) return rc;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a->dtype, convcp_dispatch_t, *a, (int)pa->peek_every, s);
}
template <class T, bool SP, bool HAS_Z> static int scancp_launch(const AumScanTmChunkVarArgs& a, int pe, aum_stream_t s) {
    const int grid = a.nseq * (a.dim / WAVE);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_stream_scan_chunk_peeks<T, SP, HAS_Z>), (scanc_var_wave<T, SP, HAS_Z, false, true>(a, wg, pe)), a, pe);
}
template <class T> static int scancp_dispatch_t(const AumScanTmChunkVarArgs& a, int pe, aum_stream_t s) {
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        return with_bool(a.z != nullptr, [&](auto hz) { return scancp_launch<T, sp, hz>(a, pe, s); }); });
}
AUM_API int aum_scan_tm_chunk_peeks(const AumScanTmChunkPeeksArgs* pa, void* stream) {
    if (!pa) return AUM_E_NULL;
    const AumScanTmChunkVarArgs* a = &pa->base;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = scan_stream_check(*a, &var, pa->peek_every >= 1, a->total, AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED, true, a->nseq, false)) return rc;
    const AumScanTmChunkVarArgs k = scan_tm_fwd_resolve(*a);
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(k.dtype, scancp_dispatch_t, k, (int)pa->peek_every, s);
}

// ---- timeline training (stream_train_kernels.h): the peek-row scan forward with state checkpoints, and the adjoints of both operators.
// No pool: for the shared operand checks the cache pointer is the checkpoint / workspace buffer (non-NULL, aligned alike) ----
#ifndef AUM_EMU
template <class T, bool SP, bool HAS_Z> AUM_GLOBAL void k_scanp_fwd_ckpt(AumScanTmChunkVarArgs a, float* ckpt, int pe) {
    scanp_fwd_wave<T, SP, HAS_Z>(a, ckpt, (int)blockIdx.x, pe);
}
template <class T, int SPM, bool HAS_Z> AUM_GLOBAL void k_scanp_bwd(AumScanTmChunkVarArgs a, const float* ckpt, ScanpBwdOuts w, int pe) {
    scanp_bwd_wave<T, SPM, HAS_Z>(a, ckpt, w, (int)blockIdx.x, pe);
}
template <class T, bool SILU> AUM_GLOBAL void k_convp_bwd(ConvpBwdArgs a) { convp_bwd_wave<T, SILU>(a, (int)blockIdx.x); }
#endif
static bool scanp_dims_ok(int64_t total, int64_t nseq, int64_t dim, int64_t dstate) { return total > 0 && nseq > 0 && dim > 0 && dstate > 0; }
AUM_API int64_t aum_scan_tm_peeks_ckpt_bytes(int32_t total, int32_t nseq, int32_t dim, int32_t dstate) {
    return scanp_dims_ok(total, nseq, dim, dstate) ? scanp_ck_slots(total, nseq) * dim * dstate * (int64_t)sizeof(float) : 0;
}
AUM_API int64_t aum_scan_tm_peeks_bwd_workspace_bytes(int32_t total, int32_t nseq, int32_t dim, int32_t dstate) {
    if (!scanp_dims_ok(total, nseq, dim, dstate)) return 0;
    return ((int64_t)(dim / WAVE) * total * 2 * dstate + (int64_t)nseq * dim * (dstate + 2)) * (int64_t)sizeof(float);
}
AUM_API int64_t aum_conv1d_tm_peeks_bwd_workspace_bytes(int32_t nseq, int32_t dim, int32_t width) {
    return nseq > 0 && dim > 0 && width > 0 ? (int64_t)nseq * dim * (width + 1) * (int64_t)sizeof(float) : 0;
}
// what the forward and the backward share behind scan_stream_check: the 32-bit cursors of a sequence's checkpoints and of the dB | dC rows
static bool scanp_cursors_ok(const AumScanTmChunkVarArgs& a) {
    const int64_t lim = ((int64_t)1 << 31) - 1;
    return ((int64_t)a.total / STREAM_UB + 1) * a.dim * a.dstate * 4 <= lim && ((int64_t)a.total + 1) * 2 * a.dstate * 4 <= lim;
}
template <class T, bool SP, bool HAS_Z> static int scanp_fwd_launch(const AumScanTmChunkVarArgs& a, float* ckpt, int pe, aum_stream_t s) {
    const int grid = a.nseq * (a.dim / WAVE);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_scanp_fwd_ckpt<T, SP, HAS_Z>), (scanp_fwd_wave<T, SP, HAS_Z>(a, ckpt, wg, pe)), a, ckpt, pe);
}
template <class T> static int scanp_fwd_dispatch_t(const AumScanTmChunkVarArgs& a, float* ckpt, int pe, aum_stream_t s) {
    return with_bool((a.flags & AUM_SCAN_SOFTPLUS) != 0, [&](auto sp) {
        return with_bool(a.z != nullptr, [&](auto hz) { return scanp_fwd_launch<T, sp, hz>(a, ckpt, pe, s); }); });
}
AUM_API int aum_scan_tm_peeks_fwd_ckpt(const AumScanTmPeeksFwdArgs* pa, void* stream) {
    if (!pa) return AUM_E_NULL;
    if (!pa->ckpt) return AUM_E_NULL;
    AumScanTmChunkVarArgs a = pa->base;
    a.state = pa->ckpt;
    a.state_indices = nullptr;
    a.nrows = a.nseq;
    const StreamVar var = {a.cu_seqlens, nullptr, a.total, a.nseq, a.nrows};
    if (const int rc = scan_stream_check(a, &var, pa->peek_every >= 1, a.total, AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED, scanp_cursors_ok(a), a.nseq, false)) return rc;
    if (pa->ckpt_bytes < aum_scan_tm_peeks_ckpt_bytes(a.total, a.nseq, a.dim, a.dstate)) return AUM_E_WORKSPACE;
    const AumScanTmChunkVarArgs k = scan_tm_fwd_resolve(a);
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(k.dtype, scanp_fwd_dispatch_t, k, pa->ckpt, (int)pa->peek_every, s);
}
template <class T, int SPM, bool HAS_Z> static int scanp_bwd_launch(const AumScanTmChunkVarArgs& a, const float* ckpt, const ScanpBwdOuts& w, int pe, aum_stream_t s) {
    const int grid = a.nseq * (a.dim / WAVE);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_scanp_bwd<T, SPM, HAS_Z>), (scanp_bwd_wave<T, SPM, HAS_Z>(a, ckpt, w, wg, pe)), a, ckpt, w, pe);
}
template <class T> static int scanp_bwd_dispatch_t(const AumScanTmChunkVarArgs& a, const float* ckpt, const ScanpBwdOuts& w, int pe, aum_stream_t s) {
    const int spm = (a.flags & AUM_SCAN_DELTA_ACTIVATED) ? SCANP_ACTIVATED : (a.flags & AUM_SCAN_SOFTPLUS) ? SCANP_SOFTPLUS : SCANP_RAW;
    return with_int<SCANP_RAW, SCANP_SOFTPLUS, SCANP_ACTIVATED>(spm, [&](auto m) {
        return with_bool(a.z != nullptr, [&](auto hz) { return scanp_bwd_launch<T, m, hz>(a, ckpt, w, pe, s); }); });
}
AUM_API int aum_scan_tm_peeks_bwd(const AumScanTmPeeksBwdArgs* pa, void* stream) {
    if (!pa) return AUM_E_NULL;
    if (!pa->ckpt || !pa->du || !pa->ddelta || !pa->workspace || (pa->base.z && !pa->dz)) return AUM_E_NULL;
    AumScanTmChunkVarArgs a = pa->base;
    a.state = const_cast<float*>(pa->ckpt);
    a.state_indices = nullptr;
    a.nrows = a.nseq;
    const StreamVar var = {a.cu_seqlens, nullptr, a.total, a.nseq, a.nrows};
    const uint32_t allowed = AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED;
    if (const int rc = scan_stream_check(a, &var, pa->peek_every >= 1, a.total, allowed, scanp_cursors_ok(a), a.nseq, false)) return rc;
    AumScanTmChunkVarArgs g = a;            // the gradients of the rows under the same rules as the rows
    g.u = pa->du; g.delta = pa->ddelta; g.z = a.z ? pa->dz : nullptr; g.state = pa->workspace;
    g.u_ts = pa->du_ts; g.delta_ts = pa->ddelta_ts; g.z_ts = a.z ? pa->dz_ts : 0;
    if (const int rc = scan_stream_check(g, &var, true, a.total, allowed, true, a.nseq, false)) return rc;
    if (pa->ckpt_bytes < aum_scan_tm_peeks_ckpt_bytes(a.total, a.nseq, a.dim, a.dstate)) return AUM_E_WORKSPACE;
    if (pa->workspace_bytes < aum_scan_tm_peeks_bwd_workspace_bytes(a.total, a.nseq, a.dim, a.dstate)) return AUM_E_WORKSPACE;
    ScanpBwdOuts w;
    w.du = pa->du; w.ddelta = pa->ddelta; w.dz = pa->dz;
    w.du_ts = pa->du_ts; w.ddelta_ts = pa->ddelta_ts; w.dz_ts = pa->dz_ts;
    w.dbc_part = pa->workspace;
    w.dA_part = w.dbc_part + (int64_t)(a.dim / WAVE) * a.total * 2 * a.dstate;
    w.dD_part = w.dA_part + (int64_t)a.nseq * a.dim * a.dstate;
    w.dbias_part = w.dD_part + (int64_t)a.nseq * a.dim;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a.dtype, scanp_bwd_dispatch_t, a, pa->ckpt, w, (int)pa->peek_every, s);
}
template <class T, bool SILU> static int convp_bwd_launch(const ConvpBwdArgs& a, int nseq, aum_stream_t s) {
    const int grid = nseq * convt_cblocks<T, true>(a.dim);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convp_bwd<T, SILU>), (convp_bwd_wave<T, SILU>(a, wg)), a);
}
template <class T> static int convp_bwd_dispatch_t(const ConvpBwdArgs& a, int nseq, bool silu, aum_stream_t s) {
    return with_bool(silu, [&](auto sl) { return convp_bwd_launch<T, sl>(a, nseq, s); });
}
AUM_API int aum_conv1d_tm_peeks_bwd(const AumConvTmPeeksBwdArgs* pa, void* stream) {
    if (!pa) return AUM_E_NULL;
    if (!pa->dy || !pa->workspace) return AUM_E_NULL;
    AumConvTmChunkVarArgs c = {};           // (x, dx) and (dy, dx) under the rules of the forward's (x, y)
    c.x = pa->x; c.conv_state = pa->workspace; c.weight = pa->weight; c.bias = pa->bias; c.y = pa->dx;
    c.cu_seqlens = pa->cu_seqlens; c.x_ts = pa->x_ts; c.y_ts = pa->dx_ts;
    c.total = pa->total; c.nseq = pa->nseq; c.nrows = pa->nseq; c.dim = pa->dim; c.width = pa->width; c.dtype = pa->dtype; c.flags = pa->flags;
    const StreamVar var = {c.cu_seqlens, nullptr, c.total, c.nseq, c.nrows};
    const uint32_t allowed = AUM_CONV_SILU;
    if (const int rc = conv_stream_check(c, &var, pa->peek_every >= 1, c.total, 0, allowed, ((uintptr_t)pa->workspace & 15) == 0, 2 * (int64_t)c.nseq)) return rc;
    c.x = pa->dy; c.x_ts = pa->dy_ts;
    if (const int rc = conv_stream_check(c, &var, true, c.total, 0, allowed, true, 0)) return rc;
    if (pa->workspace_bytes < aum_conv1d_tm_peeks_bwd_workspace_bytes(c.nseq, c.dim, c.width)) return AUM_E_WORKSPACE;
    ConvpBwdArgs k;
    k.x = pa->x; k.dy = pa->dy; k.weight = pa->weight; k.bias = pa->bias; k.dx = pa->dx;
    k.dw_part = pa->workspace;
    k.db_part = pa->bias ? pa->workspace + (int64_t)c.nseq * c.dim * c.width : nullptr;
    k.cu_seqlens = pa->cu_seqlens;
    k.x_ts = pa->x_ts; k.dy_ts = pa->dy_ts; k.dx_ts = pa->dx_ts;
    k.total = c.total; k.dim = c.dim; k.width = c.width; k.pe = pa->peek_every;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(c.dtype, convp_bwd_dispatch_t, k, (int)c.nseq, (pa->flags & AUM_CONV_SILU) != 0, s);
}

// ---- conv -> x/dt projections -> scan of packed sessions in one launch (stream_block_kernels.h) ----
#ifdef AUM_EMU
// the operands as the lane-array build's three entry points take them: its aum_xdt_tm_fwd is a plain loop that writes the raw product, so
// the bias and the softplus are the scan's here (the same function of the same values, rounded in another place than on the device)
static void sb_split(const AumStreamBlockArgs& a, AumConvTmChunkVarArgs& c, AumXdtArgs& g, AumScanTmChunkVarArgs& k) {
    const bool peek = (a.flags & AUM_STREAM_PEEK_LAST) != 0;     // handed on to the conv and the scan; the projections take every row
    const SbScratch so = sb_scratch(a.total, a.dim, a.ncols);
    char* sc = static_cast<char*>(a.scratch);
    void *xc = sc + so.xc * 2, *delta = sc + so.delta * 2, *x_dbl = sc + so.x_dbl * 2;
    c = {};
    c.x = a.x; c.conv_state = a.conv_state; c.weight = a.conv_weight; c.bias = a.conv_bias; c.y = xc;
    c.cu_seqlens = a.cu_seqlens; c.state_indices = a.state_indices;
    c.x_ts = a.x_ts; c.y_ts = a.dim;
    c.total = a.total; c.nseq = a.nseq; c.nrows = a.nrows; c.dim = a.dim; c.width = a.width; c.dtype = a.dtype;
    c.flags = AUM_CONV_SILU | (peek ? AUM_CONV_PEEK_LAST : 0u);
    g = {};
    g.u = xc; g.wx = a.wx; g.wdt = a.wdt; g.x_dbl = x_dbl; g.delta = delta;
    g.ntok = a.total; g.dim = a.dim; g.rank = a.rank; g.ncols = a.ncols;
    g.ldu = a.dim; g.ldwx = a.ldwx; g.ldwdt = a.ldwdt; g.ldx = a.ncols; g.ldd = a.dim; g.dtype = a.dtype;
    g.delta_bias = nullptr; g.flags = 0;
    k = {};
    k.u = xc; k.delta = delta; k.z = a.z;
    k.B = static_cast<char*>(x_dbl) + (int64_t)a.rank * 2; k.C = static_cast<char*>(x_dbl) + (int64_t)(a.rank + SCANT_N) * 2;
    k.A = a.A; k.D = a.D; k.delta_bias = a.delta_bias; k.state = a.state; k.out = a.y;
    k.cu_seqlens = a.cu_seqlens; k.state_indices = a.state_indices;
    k.u_ts = a.dim; k.delta_ts = a.dim; k.z_ts = a.z_ts; k.B_ts = a.ncols; k.C_ts = a.ncols; k.out_ts = a.y_ts;
    k.total = a.total; k.nseq = a.nseq; k.nrows = a.nrows; k.dim = a.dim; k.dstate = a.dstate; k.dtype = a.dtype;
    k.flags = AUM_SCAN_SOFTPLUS | (peek ? AUM_SCAN_PEEK_LAST : 0u);
}
#else
template <class T, bool BF16, bool PEEK> static int sb_launch(const AumStreamBlockArgs& a, aum_stream_t s) {
    return with_bool(a.rank <= 32, [&](auto one) {
        return with_int<XDT_FWD_WIDTHS>(a.ncols, [&](auto nc) {
            return AUM_LAUNCH(a.nseq, SB_NW * 64, s, (NoLds{}), (k_stream_block<T, BF16, one ? 1 : 2, nc, PEEK>), (0), a);
        });
    });
}
#endif
AUM_API int32_t aum_stream_block_max_len(void) { return SB_MAX_T; }
AUM_API int64_t aum_stream_block_scratch_bytes(int32_t total, int32_t dim, int32_t ncols) {
    if (total <= 0 || dim <= 0 || ncols <= 0) return 0;
    return sb_scratch(total, dim, ncols).total * 2;
}
// the operand check of aum_stream_block_tm (and of every block of aum_stream_layers, before its first launch)
static int stream_block_check(const AumStreamBlockArgs* a) {
    if (!a || !a->x || !a->z || !a->conv_state || !a->state || !a->conv_weight || !a->wx || !a->wdt || !a->A || !a->y || !a->scratch) return AUM_E_NULL;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = stream_var_check(&var)) return rc;
    if (a->dim <= 0 || a->width <= 0 || a->dstate <= 0 || a->rank <= 0 || a->ncols <= 0 || a->max_len <= 0 || a->ldwx < a->dim || a->ldwdt < a->rank)
        return AUM_E_SHAPE;
    if (a->dtype < 0 || a->dtype > 2) return AUM_E_DTYPE;
    if (a->dtype == AUM_F32) return AUM_E_DTYPE;                  // the projections run on the 16-bit matrix pipe only
    if (a->flags & ~(AUM_STREAM_NO_COMMIT | AUM_STREAM_PEEK_LAST)) return AUM_E_UNSUPPORTED;
    if (a->max_len > SB_MAX_T) return AUM_E_UNSUPPORTED;
    if (a->width != CONVT_W || a->dstate != SCANT_N || !scant_supported(a->dim, a->dstate)) return AUM_E_UNSUPPORTED;
    if (!aumx::xdt_fwd_shape_ok(a->ncols, a->dim) || a->rank % 8 || a->rank > 64 || a->rank + 2 * SCANT_N > a->ncols || a->ldwx % 8 || a->ldwdt % 8)
        return AUM_E_UNSUPPORTED;
    if (a->x_ts < a->dim || a->z_ts < a->dim || a->y_ts < a->dim || ((a->x_ts | a->z_ts | a->y_ts) & 7)) return AUM_E_UNSUPPORTED;
    {
        const uintptr_t ptrs = (uintptr_t)a->x | (uintptr_t)a->z | (uintptr_t)a->y | (uintptr_t)a->scratch | (uintptr_t)a->conv_weight | (uintptr_t)a->conv_bias |
                               (uintptr_t)a->wx | (uintptr_t)a->wdt | (uintptr_t)a->A | (uintptr_t)a->D | (uintptr_t)a->delta_bias | (uintptr_t)a->state |
                               (uintptr_t)a->conv_state;
        if (ptrs & 15) return AUM_E_UNSUPPORTED;
        if (a->x == a->y) return AUM_E_UNSUPPORTED;
        const int64_t lim = ((int64_t)1 << 31) - 1;               // row offsets inside a sequence are 32-bit byte cursors
        const int64_t ts = a->x_ts > a->z_ts ? (a->x_ts > a->y_ts ? a->x_ts : a->y_ts) : (a->z_ts > a->y_ts ? a->z_ts : a->y_ts);
        if ((ts + a->dim) * 2 * a->total > lim || (int64_t)a->nseq > lim) return AUM_E_UNSUPPORTED;
    }
    if (a->scratch_bytes < aum_stream_block_scratch_bytes(a->total, a->dim, a->ncols)) return AUM_E_WORKSPACE;
    return AUM_OK;
}
// the launch behind the check (aum_stream_layers has checked every block before its first launch and calls this alone)
static int stream_block_run(const AumStreamBlockArgs* a, void* stream) {
#ifdef AUM_EMU
    // the lane-array build has no matrix pipe: the three host entry points behind one another on the same operands.
    // AUM_STREAM_NO_COMMIT: the pools are advanced in copies.
    AumConvTmChunkVarArgs c;
    AumXdtArgs g;
    AumScanTmChunkVarArgs k;
    sb_split(*a, c, g, k);
    std::vector<float> cw, sw;
    if (a->flags & AUM_STREAM_NO_COMMIT) {
        cw.assign(a->conv_state, a->conv_state + (int64_t)a->nrows * a->dim * a->width);
        sw.assign(a->state, a->state + (int64_t)a->nrows * a->dim * a->dstate);
        c.conv_state = cw.data();
        k.state = sw.data();
    }
    int rc = aum_conv1d_tm_chunk_var(&c, stream);
    if (rc == AUM_OK) rc = aum_xdt_tm_fwd(&g, stream);
    if (rc == AUM_OK) rc = aum_scan_tm_chunk_var(&k, stream);
    return rc;
#else
    aum_stream_t s = (aum_stream_t)stream;
    return with_bool((a->flags & AUM_STREAM_PEEK_LAST) != 0, [&](auto peek) {
        return a->dtype == AUM_BF16 ? sb_launch<bf16_t, true, peek>(*a, s) : sb_launch<f16_t, false, peek>(*a, s); });
#endif
}
AUM_API int aum_stream_block_tm(const AumStreamBlockArgs* a, void* stream) {
    if (const int rc = stream_block_check(a)) return rc;
    return stream_block_run(a, stream);
}

// ---- packed prefill (stream_prefill_kernels.h): the backlogs of many sessions, time-parallel conv and state in / state out scan ----
#ifndef AUM_EMU
template <class T, bool SILU> AUM_GLOBAL void k_convt_prefill_var(AumConvTmPrefillVarArgs a) { convp_var_wave<T, SILU>(a, (int)blockIdx.x); }
#endif
template <class T, bool SILU> static int convpv_launch(const AumConvTmPrefillVarArgs& a, aum_stream_t s) {
    const int grid = a.nseq * convt_chunks<false>(a.max_len) * convt_cblocks<T, false>(a.dim);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_convt_prefill_var<T, SILU>), (convp_var_wave<T, SILU>(a, wg)), a);
}
template <class T> static int convpv_dispatch_t(const AumConvTmPrefillVarArgs& a, aum_stream_t s) {
    return with_bool((a.flags & AUM_CONV_SILU) != 0, [&](auto silu) { return convpv_launch<T, silu>(a, s); });
}
AUM_API int aum_conv1d_tm_prefill_var(const AumConvTmPrefillVarArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = conv_stream_check(*a, &var, a->max_len > 0, a->total, 0, AUM_CONV_SILU, a->max_len <= a->total,
                                         (int64_t)a->nseq * convt_chunks<false>(a->max_len > 0 ? a->max_len : 1)))
        return rc;
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_T(a->dtype, convpv_dispatch_t, *a, s);
}
AUM_API int64_t aum_scan_tm_fwd_state_var_carry_bytes(int32_t nseq, int32_t dim, int32_t dstate, int32_t nranges) {
    if (nseq <= 0 || dim <= 0 || nranges < 1 || nranges > AUM_SCAN_TM_MAX_SEGMENTS || !scant_supported(dim, dstate)) return 0;
    return scant_seg_carry_floats(nseq, dim, nranges, false) * (int64_t)sizeof(float);
}
AUM_API int aum_scan_tm_fwd_state_var(const AumScanTmFwdStateVarArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const StreamVar var = {a->cu_seqlens, a->state_indices, a->total, a->nseq, a->nrows};
    if (const int rc = scan_stream_check(*a, &var, a->max_len > 0 && a->range_len >= 0, a->total, AUM_SCAN_SOFTPLUS | AUM_SCAN_DELTA_ACTIVATED,
                                         a->max_len <= a->total, 0, true))
        return rc;
    const int64_t lim = ((int64_t)1 << 31) - 1;
    int nranges = 1;
    if (a->range_len > 0) {
        if (a->range_len % SCANT_CK) return AUM_E_UNSUPPORTED;
        nranges = (a->max_len + a->range_len - 1) / a->range_len;
        if (nranges > AUM_SCAN_TM_MAX_SEGMENTS) return AUM_E_UNSUPPORTED;
        if (!a->carry) return AUM_E_NULL;
        if (((uintptr_t)a->carry & 3) || a->carry_bytes < scant_seg_carry_floats(a->nseq, a->dim, nranges, false) * (int64_t)sizeof(float)) return AUM_E_WORKSPACE;
    }
    if ((int64_t)a->nseq * (a->dim / WAVE) * nranges > lim) return AUM_E_UNSUPPORTED;
    // the kernels' view: a fixed-batch argument struct whose "batch entry" b is a packed row (X_bs := X_ts); an activated delta carries
    // its bias and softplus already
    AumScanTmFwdArgs k = {};
    k.u = a->u; k.delta = a->delta; k.z = a->z; k.B = a->B; k.C = a->C;
    k.A = a->A; k.D = a->D; k.delta_bias = a->delta_bias; k.out = a->out;
    k.u_bs = k.u_ts = a->u_ts; k.delta_bs = k.delta_ts = a->delta_ts; k.z_bs = k.z_ts = a->z ? a->z_ts : 0;
    k.B_bs = k.B_ts = a->B_ts; k.C_bs = k.C_ts = a->C_ts; k.out_bs = k.out_ts = a->out_ts;
    k.batch = a->nseq; k.dim = a->dim; k.len = a->max_len; k.dstate = a->dstate; k.dtype = a->dtype; k.flags = a->flags;
    k = scan_tm_fwd_resolve(k);
    const ScanTVar v = {a->cu_seqlens, a->state_indices, a->state, a->total, a->nseq, a->nrows, a->max_len};
    aum_stream_t s = (aum_stream_t)stream;
    auto run = [&](const ScanTSeg* sg, int phase) {
        return AUM_BY_DTYPE_X(k.dtype, scan_tm_fwd_state_var, k, v, sg, phase, s);
    };
    if (a->range_len == 0) return run(nullptr, 0);
    ScanTSeg sg;
    sg.carry = a->carry;
    sg.nseg = nranges;
    sg.seg_len = a->range_len;
    sg.dir0 = 0;
    sg.ndl = 1;
    const int r = run(&sg, 3);
    if (r != AUM_OK) return r;
    return run(&sg, 0);
}

// ---- streaming log-mel (fbank_kernels.h): the new frames of many sessions from [carried tail ; hop], then the new tails ----
#ifndef AUM_EMU
__global__ __launch_bounds__(FBANK_THREADS) void k_fbank_stream(AumFbankStreamArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[FbankWLds::n];
    fbank_stream_frames_wg(a, (int)blockIdx.x, lds);
}
__global__ __launch_bounds__(FBANK_THREADS) void k_fbank_stream_tail(AumFbankStreamArgs a) { fbank_stream_tail_wg(a, (int)blockIdx.x); }
#endif
AUM_API int aum_fbank_stream_fwd(const AumFbankStreamArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const AumFbankArgs& f = a->fbank;
    if (!f.window || !f.twiddle || !f.mel_start_f || !f.mel_count_f || !f.mel_w || !a->cu_frames || !a->tail_len || !a->first_frame || !a->n_real || !a->tails)
        return AUM_E_NULL;
    if ((a->total_samples > 0 && !f.wave) || (a->total_frames > 0 && !f.out)) return AUM_E_NULL;
    const int64_t work = (int64_t)a->total_samples + a->total_frames;
    if (a->total_samples < 0 || a->total_frames < 0 || work > 0x7fffffff) return AUM_E_SHAPE;
    // the packed map: the samples and the frames of a call are its rows (a call with neither has nothing to do and is refused)
    const StreamVar var = {a->cu_samples, a->idx, (int)work, a->nseq, a->nrows};
    if (const int rc = stream_var_check(&var)) return rc;
    if (f.win <= 0 || f.shift <= 0 || f.num_mel <= 0 || f.mel_wstride <= 0 || a->cap <= 0) return AUM_E_SHAPE;
    if (f.aug || f.noise || f.padded != FBW_N || f.win > FBW_N) return AUM_E_UNSUPPORTED;
    if ((int64_t)a->cap != (int64_t)f.win + 15 * (int64_t)f.shift || a->cap > FBS_MAX_CAP) return AUM_E_UNSUPPORTED;
    const uintptr_t maps = (uintptr_t)a->cu_frames | (uintptr_t)a->tail_len | (uintptr_t)a->first_frame | (uintptr_t)a->n_real;
    if ((maps & 3) || (((uintptr_t)a->tails | (uintptr_t)f.wave | (uintptr_t)f.out) & 3)) return AUM_E_UNSUPPORTED;
    aum_stream_t s = (aum_stream_t)stream;
    if (a->total_frames > 0) {
        const int rc = AUM_LAUNCH((a->total_frames + FBW_WG_FRAMES - 1) / FBW_WG_FRAMES, FBANK_THREADS, s, (FbankWLds{}), k_fbank_stream,
                                  (fbank_stream_frames_wg(*a, wg, lds)), *a);
        if (rc != AUM_OK) return rc;
    }
    // behind the frames on the same stream: the frame waves have read the old tails before any of them is rewritten
    return AUM_LAUNCH(a->nseq, FBANK_THREADS, s, (NoLds{}), k_fbank_stream_tail, (fbank_stream_tail_wg(*a, wg)), *a);
}

// ---- park / resume (stream_park_kernels.h): the pool rows of many sessions to one record each of a blob, or back, in one launch ----
// park_check is this family's one operand check; the grid is (session, tensor, 4 KiB chunk) flattened, per_session chunks per session
#include "stream_park_kernels.h"
AUM_API int aum_stream_park(const AumParkArgs* a, void* stream) {
    int64_t per_session = 0;
    if (const int rc = park_check(a, &per_session)) return rc;
    return AUM_LAUNCH(per_session * a->n_sessions, PARK_THREADS, (aum_stream_t)stream, (NoLds{}), k_stream_park, (park_wg(*a, per_session, wg)), *a,
                      per_session);
}

// ---- a hop through all blocks in one call (stream_stack_kernels.h): add + norm + in_proj, the block above, out_proj, per layer ----
#include "stream_stack_kernels.h"
AUM_API int aum_stream_in_tm(const AumStreamInArgs* a, void* stream) {
    if (const int rc = ss_in_check(a)) return rc;
    return ss_in_run(*a, (aum_stream_t)stream);
}
AUM_API int aum_stream_out_tm(const AumStreamOutArgs* a, void* stream) {
    if (const int rc = ss_out_check(a)) return rc;
    return ss_out_run(*a, (aum_stream_t)stream);
}
AUM_API int64_t aum_stream_layers_scratch_bytes(int32_t total, int32_t d_model, int32_t dim, int32_t ncols) {
    if (total <= 0 || d_model <= 0 || dim <= 0 || ncols <= 0) return 0;
    return ss_ws(total, d_model, dim, aum_stream_block_scratch_bytes(total, dim, ncols)).total;
}
// the three argument structs of layer l as the loop hands them on: block l reads hidden / residual l - 1 and writes l (two buffers each,
// taken in turn; the call's own operands at both ends)
static void ss_layer_args(const AumStreamLayersArgs& a, const SsWs& w, int l, AumStreamInArgs& in, AumStreamBlockArgs& b, AumStreamOutArgs& out) {
    const AumStreamLayer& L = a.layers[l];
    char* ws = static_cast<char*>(a.workspace);
    const bool first = l == 0, last = l == a.depth - 1;
    in = {};
    in.hidden = first ? a.hidden : ws + w.hid[(l - 1) & 1];
    in.residual_in = first ? a.residual_in : reinterpret_cast<const float*>(ws + w.res[(l - 1) & 1]);
    in.norm_weight = L.norm_weight; in.w_in = L.w_in;
    in.residual_out = last ? a.residual_out : reinterpret_cast<float*>(ws + w.res[l & 1]);
    in.xz = ws + w.xz;
    in.hidden_ts = first ? a.hidden_ts : a.d_model; in.xz_ts = 2 * (int64_t)a.dim;
    in.total = a.total; in.d_model = a.d_model; in.dim = a.dim; in.ldw = a.d_model; in.dtype = a.dtype; in.eps = a.eps;
    b = {};
    b.x = ws + w.xz; b.z = ws + w.xz + (int64_t)a.dim * 2;
    b.conv_state = L.conv_state; b.state = L.state; b.conv_weight = L.conv_weight; b.conv_bias = L.conv_bias;
    b.wx = L.wx; b.wdt = L.wdt; b.A = L.A; b.D = L.D; b.delta_bias = L.delta_bias;
    b.y = ws + w.y; b.scratch = ws + w.block;
    b.cu_seqlens = a.cu_seqlens; b.state_indices = a.state_indices;
    b.x_ts = b.z_ts = 2 * (int64_t)a.dim; b.y_ts = a.dim; b.scratch_bytes = w.block_bytes;
    b.total = a.total; b.nseq = a.nseq; b.nrows = a.nrows; b.max_len = a.max_len;
    b.dim = a.dim; b.width = CONVT_W; b.dstate = SCANT_N; b.rank = a.rank; b.ncols = a.ncols; b.ldwx = a.ldwx; b.ldwdt = a.ldwdt;
    b.dtype = a.dtype; b.flags = a.flags;
    out = {};
    out.y = ws + w.y; out.w_out = L.w_out; out.out = last ? a.hidden_out : ws + w.hid[l & 1];
    out.y_ts = a.dim; out.out_ts = a.d_model;
    out.total = a.total; out.d_model = a.d_model; out.dim = a.dim; out.ldw = a.dim; out.dtype = a.dtype;
}
// aum_hip.stream_layers_supported states the same rules in the same order
static int stream_layers_check(const AumStreamLayersArgs* a, SsWs* wo) {
    if (!a || !a->layers || !a->hidden || !a->hidden_out || !a->residual_out || !a->workspace || !a->cu_seqlens) return AUM_E_NULL;
    if (a->depth <= 0 || a->total <= 0 || a->nseq <= 0 || a->nrows <= 0 || a->d_model <= 0 || a->dim <= 0 || a->ncols <= 0 || a->rank <= 0) return AUM_E_SHAPE;
    for (int l = 0; l < a->depth; ++l) {
        const AumStreamLayer& L = a->layers[l];
        if (!L.norm_weight || !L.w_in || !L.conv_weight || !L.wx || !L.wdt || !L.A || !L.w_out || !L.conv_state || !L.state) return AUM_E_NULL;
    }
    if (a->dtype < 0 || a->dtype > 2 || a->dtype == AUM_F32) return AUM_E_DTYPE;
    if (!ss_widths_ok(a->d_model, a->dim)) return AUM_E_UNSUPPORTED;
    if (((uintptr_t)a->workspace | (uintptr_t)a->hidden_out | (uintptr_t)a->residual_out) & 15) return AUM_E_UNSUPPORTED;
    if (a->residual_in == a->residual_out) return AUM_E_UNSUPPORTED;
    const SsWs w = ss_ws(a->total, a->d_model, a->dim, aum_stream_block_scratch_bytes(a->total, a->dim, a->ncols));
    if (a->workspace_bytes < w.total) return AUM_E_WORKSPACE;
    for (int l = 0; l < a->depth; ++l) {
        AumStreamInArgs in;
        AumStreamBlockArgs b;
        AumStreamOutArgs out;
        ss_layer_args(*a, w, l, in, b, out);
        if (const int rc = ss_in_check(&in)) return rc;
        if (const int rc = stream_block_check(&b)) return rc;
        if (const int rc = ss_out_check(&out)) return rc;
    }
    *wo = w;
    return AUM_OK;
}
AUM_API int aum_stream_layers(const AumStreamLayersArgs* a, void* stream) {
    SsWs w;
    if (const int rc = stream_layers_check(a, &w)) return rc;
    for (int l = 0; l < a->depth; ++l) {
        AumStreamInArgs in;
        AumStreamBlockArgs b;
        AumStreamOutArgs out;
        ss_layer_args(*a, w, l, in, b, out);
        if (const int rc = ss_in_run(in, (aum_stream_t)stream)) return rc;
        if (const int rc = stream_block_run(&b, stream)) return rc;
        if (const int rc = ss_out_run(out, (aum_stream_t)stream)) return rc;
    }
    return AUM_OK;
}
#endif
