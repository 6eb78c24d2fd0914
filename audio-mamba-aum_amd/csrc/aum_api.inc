// aum_api.inc -- the C-ABI entry points of include/aum_hip.h: argument validation, kernel selection
// (element type, steps-per-lane K, direction mode) and launch.  Included by aum_hip.hip (device build)
// and by tests/emu/aum_emu.cpp (lane-array build, tests only) so both share one dispatcher.
//
// Every kernel is started by AUM_LAUNCH (launch.h): grid, workgroup size, stream, the kernel's LDS, the k_* entry, its workgroup body
// and the entry's arguments -- a loop of the body over the grid in the lane-array build.  A kernel's LDS is an Lds<> type stated once,
// next to its entry.  Runtime flags, mode / K and the dtype reach template parameters through with_bool / with_int / by_dtype.
//
// AUM_DTYPE_ONLY (optional, 0/1/2) restricts a translation unit to one activation dtype so the device
// library can be compiled as parallel objects; AUM_API_PART selects which entry points a TU defines.

#include "conv_norm_kernels.h"
#include "scan_kernels.h"
#include "scan_wg_kernels.h"
#include "scan_half_kernels.h"
#include "scan_row_kernels.h"
#include "fbank_kernels.h"
#include "stft_kernels.h"
#include "proj_kernels.h"
#include "frontend_kernels.h"
#include "conv_rows_kernels.h"
#include "launch.h"
#ifndef AUM_API_PART
#define AUM_API_PART 0
#endif

namespace aum {

#ifdef AUM_EMU
#define AUM_GLOBAL
#else
#define AUM_GLOBAL __global__ __launch_bounds__(64)
#endif

#ifndef AUM_SCANWG_FWD_MINW
#define AUM_SCANWG_FWD_MINW 4      // waves per SIMD the forward scan is compiled for (<= 128 VGPRs: two 8-wave workgroups per CU)
#endif
// ---- kernel entries and their LDS --------------------------------------------------------------
typedef Lds<float, SCAN_LDS_FLOATS> ScanLds;
typedef Lds<float, CONV_LDS_FLOATS> ConvLds;
template <int K, int TAIL, bool CT = false> using ScanWgFwdLds = Lds<float, scanwg_fwd_lds_floats<K, TAIL, CT>()>;
template <int K, int TAIL> using ScanWgBwdLds = Lds<float, scanwg_bwd_lds_floats<K, TAIL>()>;
template <int TAIL> using ScanHBwdLds = Lds<float, scanh_bwd_lds_floats<TAIL>()>;
template <int TAIL> using ScanHChunkedLds = Lds<float, scanh_chunked_lds_floats<TAIL>()>;
typedef Lds<float, scanr_fwd_lds_floats()> ScanRFwdLds;
typedef Lds<float, scanr_bwd_lds_floats()> ScanRBwdLds;
template <int NCH> using NormBwdVecLds = Lds<float, (NORM_BWD_NW - 1) * NCH * 512>;
#ifndef AUM_EMU
template <class T, int K, int MODE> AUM_GLOBAL void k_scan_fwd(AumScanFwdArgs a) {
    __shared__ float lds[ScanLds::n];
    scan_fwd_wave<T, K, MODE>(a, (int)blockIdx.x, lds);
}
template <class T, int K, int MODE> AUM_GLOBAL void k_scan_bwd(AumScanBwdArgs a) {
    __shared__ float lds[ScanLds::n];
    scan_bwd_wave<T, K, MODE>(a, (int)blockIdx.x, lds);
}
template <class T, int K, int TAIL, int MODE> __global__ __launch_bounds__(SCANWG_NW * 64, AUM_SCANWG_FWD_MINW) void k_scanwg_fwd(AumScanFwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanWgFwdLds<K, TAIL>::n];
    scanwg_fwd<T, K, TAIL, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int MODE> __global__ __launch_bounds__(SCANWG_NW * 64, AUM_SCANWG_FWD_MINW) void k_scanwg_fwd_ct(AumScanFwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanWgFwdLds<8, 1, true>::n];
    scanwg_fwd_ct<T, 8, 1, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int K, int TAIL, int MODE> __global__ __launch_bounds__(SCANWG_NW * 64) void k_scanwg_bwd(AumScanBwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanWgBwdLds<K, TAIL>::n];
    scanwg_bwd<T, K, TAIL, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int TAIL, int MODE> __global__ __launch_bounds__(scanh_nw(MODE) * 64) void k_scanh_bwd(AumScanBwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanHBwdLds<TAIL>::n];
    scanh_bwd<T, TAIL, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int TAIL, int MODE> __global__ __launch_bounds__(SCANH_CH_NW * 64) void k_scanh_bwd_chunked(AumScanBwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanHChunkedLds<TAIL>::n];
    scanh_bwd_chunked<T, TAIL, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int MODE> __global__ __launch_bounds__(SCANR_FWD_NW * 64, AUM_SCANR_FWD_MINW) void k_scanr_fwd(AumScanFwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanRFwdLds::n];
    scanr_fwd<T, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T, int MODE> __global__ __launch_bounds__(scanr_bwd_nw(MODE) * 64) void k_scanr_bwd(AumScanBwdArgs a, int rows_per_wg) {
    __shared__ __attribute__((aligned(16))) float lds[ScanRBwdLds::n];
    scanr_bwd<T, MODE>(a, (int)blockIdx.x, lds, rows_per_wg);
}
template <class T> AUM_GLOBAL void k_conv_fwd(AumConvArgs a) { conv_fwd_wave<T>(a, (int)blockIdx.x); }
template <class T> AUM_GLOBAL void k_conv_bwd(AumConvArgs a) {
    __shared__ float lds[ConvLds::n];
    conv_bwd_wave<T>(a, (int)blockIdx.x, lds);
}
template <class T, bool REV> AUM_GLOBAL void k_conv4_fwd(AumConvArgs a) { conv4_fwd_wave<T, REV>(a, (int)blockIdx.x); }
template <class T, bool REV> AUM_GLOBAL void k_conv4_bwd(AumConvArgs a) { conv4_bwd_wave<T, REV>(a, (int)blockIdx.x); }
template <class T, bool REV> AUM_GLOBAL void k_conv4_rows_fwd(AumConvArgs a) { conv4_rows_fwd_wave<T, REV>(a, (int)blockIdx.x); }
template <class T, bool REV> AUM_GLOBAL void k_conv4_rows_bwd(AumConvArgs a) { conv4_rows_bwd_wave<T, REV>(a, (int)blockIdx.x); }
template <class TX, class TR, int NCH> AUM_GLOBAL void k_norm_fwd_vec(AumNormArgs a) { rmsnorm_fwd_vec<TX, TR, NCH>(a, (int)blockIdx.x); }
template <class TX, class TR, int NCH> __global__ __launch_bounds__(NORM_BWD_NW * 64) void k_norm_bwd_vec(AumNormArgs a, int n_waves) {
    __shared__ __attribute__((aligned(16))) float lds[NormBwdVecLds<NCH>::n];
    rmsnorm_bwd_vec<TX, TR, NCH>(a, (int)blockIdx.x, n_waves, lds);
}
template <class TX, class TR> AUM_GLOBAL void k_norm_fwd(AumNormArgs a) { rmsnorm_fwd_wave<TX, TR>(a, (int)blockIdx.x); }
template <class TX, class TR> AUM_GLOBAL void k_norm_bwd(AumNormArgs a, int n_partials) {
    extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
    rmsnorm_bwd_wave<TX, TR>(a, (int)blockIdx.x, n_partials, dyn_lds);
}
// the same four with a per-sample factor on x (aum_rmsnorm_drop_fwd / _bwd)
template <class TX, class TR, int NCH> AUM_GLOBAL void k_norm_drop_fwd_vec(AumNormArgs a, RowScale sc) { rmsnorm_fwd_vec<TX, TR, NCH>(a, (int)blockIdx.x, sc); }
template <class TX, class TR, int NCH> __global__ __launch_bounds__(NORM_BWD_NW * 64) void k_norm_drop_bwd_vec(AumNormArgs a, int n_waves, RowScale sc) {
    __shared__ __attribute__((aligned(16))) float lds[NormBwdVecLds<NCH>::n];
    rmsnorm_bwd_vec<TX, TR, NCH>(a, (int)blockIdx.x, n_waves, lds, sc);
}
template <class TX, class TR> AUM_GLOBAL void k_norm_drop_fwd(AumNormArgs a, RowScale sc) { rmsnorm_fwd_wave<TX, TR>(a, (int)blockIdx.x, sc); }
template <class TX, class TR> AUM_GLOBAL void k_norm_drop_bwd(AumNormArgs a, int n_partials, RowScale sc) {
    extern __shared__ __attribute__((aligned(16))) float dyn_lds[];
    rmsnorm_bwd_wave<TX, TR>(a, (int)blockIdx.x, n_partials, dyn_lds, sc);
}
// add + RMSNorm + mean over a sample's rows (aum_rmsnorm_pool_fwd / _bwd)
template <class TX, int NCH> __global__ __launch_bounds__(NORM_BWD_NW * 64) void k_norm_pool_fwd_vec(AumNormPoolArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[NormBwdVecLds<NCH>::n];
    rmsnorm_pool_fwd_vec<TX, float, NCH>(a, (int)blockIdx.x, lds);
}
template <class TX> AUM_GLOBAL void k_norm_pool_finish(AumNormPoolArgs a) { rmsnorm_pool_finish<TX>(a, (int)blockIdx.x); }
template <class TX, int NCH> __global__ __launch_bounds__(NORM_BWD_NW * 64) void k_norm_pool_bwd_vec(AumNormArgs a, int n_waves, DyPooled g) {
    __shared__ __attribute__((aligned(16))) float lds[NormBwdVecLds<NCH>::n];
    rmsnorm_bwd_vec<TX, float, NCH, NoRowScale, DyPooled>(a, (int)blockIdx.x, n_waves, lds, NoRowScale{}, g);
}
#if AUM_API_PART == 3 || AUM_API_PART == 0
AUM_GLOBAL void k_selftest_sum32(const float* in, float* out) {
    vf v[32], w[16];
    for (int k = 0; k < 32; ++k) v[k] = in[k * 64 + threadIdx.x];
    for (int k = 0; k < 16; ++k) w[k] = v[k];
    out[64 + threadIdx.x] = wave_sum16(w);
    out[threadIdx.x] = wave_sum32(v);
}
AUM_GLOBAL void k_selftest_scan(const float* in, float* out, int rev) {
    vf P = in[threadIdx.x], S = in[64 + threadIdx.x];
    if (rev) wave_scan_affine<true>(P, S); else wave_scan_affine<false>(P, S);
    out[threadIdx.x] = P;
    out[64 + threadIdx.x] = S;
}
#endif
#endif

// ---- steps-per-lane selection -----------------------------------------------------------------
// generic single-wave kernels (dstate > 16, or AUM_SCAN_GENERIC)
static const int kScanK[] = {1, 4, 9, 16};
constexpr int kScanKCount = 4;
constexpr int kScanMaxK = 16;
// workgroup kernels: odd K only (lane stride K words in the LDS tiles is then bank-conflict free)
static const int kScanWgK[] = {1, 3, 5, 7, 9};
constexpr int kScanWgKCount = 5;

struct ScanPlan { int K; int nchunks; int tail; };
static ScanPlan scan_plan(int len) {
    ScanPlan best = {kScanMaxK, (len + WAVE * kScanMaxK - 1) / (WAVE * kScanMaxK), 0};
    if (len <= WAVE * kScanMaxK) {
        for (int i = 0; i < kScanKCount; ++i)
            if (WAVE * kScanK[i] >= len) { best.K = kScanK[i]; best.nchunks = 1; break; }
        return best;
    }
    long best_cost = (long)best.nchunks * WAVE * best.K;
    for (int i = kScanKCount - 1; i >= 0; --i) {
        const int K = kScanK[i];
        const int nc = (len + WAVE * K - 1) / (WAVE * K);
        const long cost = (long)nc * WAVE * K + 64L * nc;   // small per-chunk overhead term
        if (cost < best_cost) { best_cost = cost; best.K = K; best.nchunks = nc; }
    }
    return best;
}

static ScanPlan scanwg_plan(int len) {
    // 64K+1 rows (AuM: 64 or 512 patches + the cls token): K main slots per lane + one tail slot on the last lane
    if (len == WAVE * 8 + 1) return ScanPlan{8, 1, 1};
    if (len == WAVE * 1 + 1) return ScanPlan{1, 1, 1};
    ScanPlan best = {SCANWG_MAX_K, (len + WAVE * SCANWG_MAX_K - 1) / (WAVE * SCANWG_MAX_K), 0};
    if (len <= WAVE * SCANWG_MAX_K) {
        for (int i = 0; i < kScanWgKCount; ++i)
            if (WAVE * kScanWgK[i] >= len) { best.K = kScanWgK[i]; best.nchunks = 1; break; }
        return best;
    }
    long best_cost = (long)best.nchunks * (WAVE * best.K + 32);
    for (int i = kScanWgKCount - 1; i >= 0; --i) {
        const int K = kScanWgK[i];
        const int nc = (len + WAVE * K - 1) / (WAVE * K);
        const long cost = (long)nc * (WAVE * K + 32);
        if (cost < best_cost) { best_cost = cost; best.K = K; best.nchunks = nc; }
    }
    return best;
}
// rows per workgroup: 64 when that still gives every CU a few workgroups, fewer rows for small batches
static int scanwg_rows(int batch, int dim) {
    int rows = SCANWG_MAX_ROWS;
    while (rows > 2 * SCANWG_NW && (long)batch * ((dim + rows - 1) / rows) < 1024) rows /= 2;
    return rows;
}

// forward over rows of 512*m + 1 steps in 512-step chunks (scanwg_fwd_ct): replaces the <5,0> x 13-chunk plan
// scanwg_plan makes for L = 4097.  Rows per workgroup sized to the 2 x 256 workgroup slots of the chip.
static bool scanwg_ct_selected(int len, int dstate, int mode, uint32_t flags) {
    return mode != 2 && !(flags & AUM_SCAN_ROWPAIR) && len > 1024 && (len & 511) == 1 && dstate <= SCANWG_MAX_N;
}
#ifndef AUM_SCANWG_CT_ROWS
#define AUM_SCANWG_CT_ROWS 0      // > 0: forced row count (sweeps)
#endif
static int scanwg_ct_rows(int batch, int dim) {
    (void)batch; (void)dim;
    // two workgroups per CU: as for the L = 513 row forward, MORE, shorter workgroups win (one's tile loads and row prologues
    // overlap the other's state loops).  B = 8, L = 4097, one direction: 16 / 32 / 48 / 64 rows = 0.427 / 0.486 / 0.483 / 0.626 ms
    return AUM_SCANWG_CT_ROWS ? AUM_SCANWG_CT_ROWS : 2 * SCANWG_NW;
}

static int scan_rows_grid(int batch, int dim, int rows) { return batch * ((dim + rows - 1) / rows); }
template <class T, int K, int TAIL, int MODE> static int launch_scanwg_fwd(const AumScanFwdArgs& a, int rows, aum_stream_t s) {
    return AUM_LAUNCH(scan_rows_grid(a.batch, a.dim, rows), SCANWG_NW * 64, s, (ScanWgFwdLds<K, TAIL>{}), (k_scanwg_fwd<T, K, TAIL, MODE>),
                      (scanwg_fwd<T, K, TAIL, MODE>(a, wg, lds, rows)), a, rows);
}
// rows of 512*m + 1 steps (long-form clips), one direction: <8,1> geometry walked in 512-step chunks
template <class T, int MODE> static int launch_scanwg_fwd_ct(const AumScanFwdArgs& a, int rows, aum_stream_t s) {
    return AUM_LAUNCH(scan_rows_grid(a.batch, a.dim, rows), SCANWG_NW * 64, s, (ScanWgFwdLds<8, 1, true>{}), (k_scanwg_fwd_ct<T, MODE>),
                      (scanwg_fwd_ct<T, 8, 1, MODE>(a, wg, lds, rows)), a, rows);
}
template <class T, int K, int TAIL, int MODE> static int launch_scanwg_bwd(const AumScanBwdArgs& a, int rows, aum_stream_t s) {
    const int grid = scan_rows_grid(a.batch, a.dim, rows);
    if constexpr (K == 8 && TAIL == 1) {      // the AuM row shape: one row per wave, half-packed slots (scan_half_kernels.h)
        if (scanh_selected(K, TAIL, (a.len + ScanGeo<K, TAIL>::S - 1) / ScanGeo<K, TAIL>::S, a.len, a.dstate, a.flags))
            return AUM_LAUNCH(grid, scanh_nw(MODE) * 64, s, (ScanHBwdLds<TAIL>{}), (k_scanh_bwd<T, TAIL, MODE>),
                              (scanh_bwd<T, TAIL, MODE>(a, wg, lds, rows)), a, rows);
    }
    return AUM_LAUNCH(grid, SCANWG_NW * 64, s, (ScanWgBwdLds<K, TAIL>{}), (k_scanwg_bwd<T, K, TAIL, MODE>),
                      (scanwg_bwd<T, K, TAIL, MODE>(a, wg, lds, rows)), a, rows);
}

// long rows of 512*m (+1) steps, one direction: one row per wave, chunked (scan_half_kernels.h)
template <class T, int TAIL, int MODE> static int launch_scanh_chunked(const AumScanBwdArgs& a, int rows, aum_stream_t s) {
    return AUM_LAUNCH(scan_rows_grid(a.batch, a.dim, rows), SCANH_CH_NW * 64, s, (ScanHChunkedLds<TAIL>{}), (k_scanh_bwd_chunked<T, TAIL, MODE>),
                      (scanh_bwd_chunked<T, TAIL, MODE>(a, wg, lds, rows)), a, rows);
}

// the L = 513 row kernels (scan_row_kernels.h); plan marker {8, 1, SCANR_PLAN_TAIL}
constexpr int SCANR_PLAN_TAIL = 2;
template <class T, int MODE> static int launch_scanr_fwd(const AumScanFwdArgs& a, int rows, aum_stream_t s) {
    return AUM_LAUNCH(scan_rows_grid(a.batch, a.dim, rows), SCANR_FWD_NW * 64, s, (ScanRFwdLds{}), (k_scanr_fwd<T, MODE>),
                      (scanr_fwd<T, MODE>(a, wg, lds, rows)), a, rows);
}
template <class T, int MODE> static int launch_scanr_bwd(const AumScanBwdArgs& a, int rows, aum_stream_t s) {
    return AUM_LAUNCH(scan_rows_grid(a.batch, a.dim, rows), scanr_bwd_nw(MODE) * 64, s, (ScanRBwdLds{}), (k_scanr_bwd<T, MODE>),
                      (scanr_bwd<T, MODE>(a, wg, lds, rows)), a, rows);
}

template <class T, int K, int MODE> static int launch_scan_fwd(const AumScanFwdArgs& a, int grid, aum_stream_t s) {
    return AUM_LAUNCH(grid, 64, s, (ScanLds{}), (k_scan_fwd<T, K, MODE>), (scan_fwd_wave<T, K, MODE>(a, wg, lds)), a);
}
template <class T, int K, int MODE> static int launch_scan_bwd(const AumScanBwdArgs& a, int grid, aum_stream_t s) {
    return AUM_LAUNCH(grid, 64, s, (ScanLds{}), (k_scan_bwd<T, K, MODE>), (scan_bwd_wave<T, K, MODE>(a, wg, lds)), a);
}

// plan.K (generic kernels) and plan.K * 2 + plan.tail (workgroup kernels) into template parameters
template <class F> static int with_scan_k(int K, F&& f) { return with_int<1, 4, 9, 16>(K, f); }
template <class F> static int with_scanwg_kt(const ScanPlan& plan, F&& f) {
    return with_int<2, 3, 6, 10, 14, 17, 18>(plan.K * 2 + plan.tail, f);
}

// grid < 0 selects the workgroup kernels with rows_per_wg = -grid
// mode: 0 forward, 1 reverse, anything else the bidirectional kernels (2)
template <class T> static int scan_fwd_t(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) {
    if (mode != 0 && mode != 1) mode = 2;
    if (grid < 0 && plan.tail == SCANR_PLAN_TAIL) return with_int<0, 1, 2>(mode, [&](auto m) { return launch_scanr_fwd<T, m>(a, -grid, s); });
    if (grid < 0 && plan.K == 8 && plan.nchunks > 1)      // the plan aum_selective_scan_fwd makes for scanwg_ct_selected rows
        return with_int<0, 1>(mode, [&](auto m) { return launch_scanwg_fwd_ct<T, m>(a, -grid, s); });
    return with_int<0, 1, 2>(mode, [&](auto m) {
        if (grid < 0) return with_scanwg_kt(plan, [&](auto kt) { return launch_scanwg_fwd<T, kt / 2, kt % 2, m>(a, -grid, s); });
        return with_scan_k(plan.K, [&](auto k) { return launch_scan_fwd<T, k, m>(a, grid, s); });
    });
}
template <class T> static int scan_bwd_t(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) {
    if (mode != 0 && mode != 1) mode = 2;
    if (grid < 0 && plan.tail == SCANR_PLAN_TAIL) return with_int<0, 1, 2>(mode, [&](auto m) { return launch_scanr_bwd<T, m>(a, -grid, s); });
    if (grid < 0 && plan.K == 8 && plan.nchunks > 1)      // the plan aum_selective_scan_bwd makes for scanh_chunked_selected rows
        return with_int<0, 1>(mode, [&](auto m) { return with_int<0, 1>(plan.tail ? 1 : 0, [&](auto t) { return launch_scanh_chunked<T, t, m>(a, -grid, s); }); });
    return with_int<0, 1, 2>(mode, [&](auto m) {
        if (grid < 0) return with_scanwg_kt(plan, [&](auto kt) { return launch_scanwg_bwd<T, kt / 2, kt % 2, m>(a, -grid, s); });
        return with_scan_k(plan.K, [&](auto k) { return launch_scan_bwd<T, k, m>(a, grid, s); });
    });
}

#if defined(AUM_DTYPE_ONLY)
#define AUM_HAS_DTYPE(d) ((d) == AUM_DTYPE_ONLY)
#else
#define AUM_HAS_DTYPE(d) 1
#endif

// per-dtype workers; when the library is built as several objects each object defines only its own
int scan_fwd_f32(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);
int scan_fwd_bf16(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);
int scan_fwd_f16(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);
int scan_bwd_f32(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);
int scan_bwd_bf16(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);
int scan_bwd_f16(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s);

#if AUM_API_PART == 1 || AUM_API_PART == 0
#if AUM_HAS_DTYPE(0)
int scan_fwd_f32(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_fwd_t<float>(a, plan, mode, grid, s); }
#endif
#if AUM_HAS_DTYPE(1)
int scan_fwd_bf16(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_fwd_t<bf16_t>(a, plan, mode, grid, s); }
#endif
#if AUM_HAS_DTYPE(2)
int scan_fwd_f16(const AumScanFwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_fwd_t<f16_t>(a, plan, mode, grid, s); }
#endif
#endif
#if AUM_API_PART == 2 || AUM_API_PART == 0
#if AUM_HAS_DTYPE(0)
int scan_bwd_f32(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_bwd_t<float>(a, plan, mode, grid, s); }
#endif
#if AUM_HAS_DTYPE(1)
int scan_bwd_bf16(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_bwd_t<bf16_t>(a, plan, mode, grid, s); }
#endif
#if AUM_HAS_DTYPE(2)
int scan_bwd_f16(const AumScanBwdArgs& a, ScanPlan plan, int mode, int grid, aum_stream_t s) { return scan_bwd_t<f16_t>(a, plan, mode, grid, s); }
#endif
#endif


// ---- skinny projections (MFMA), AUM_API_PART 4: kernels + shape dispatch, one object per 16-bit dtype ------------
int proj_bf16(const AumProjArgs& a, bool bwd, aum_stream_t s);
int proj_f16(const AumProjArgs& a, bool bwd, aum_stream_t s);
int projw_bf16(const AumProjWArgs& a, int chunk, aum_stream_t s);
int projw_f16(const AumProjWArgs& a, int chunk, aum_stream_t s);
#if AUM_API_PART == 4 || AUM_API_PART == 0
typedef Lds<uint16_t, PJ_LDS_ELEMS> ProjLds;
typedef Lds<uint16_t, PJW_LDS_ELEMS> ProjWLds;
#ifndef AUM_EMU
template <class T, int NCB, bool TWO> __global__ __launch_bounds__(PJ_NW * 64) void k_proj_fwd(AumProjArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[ProjLds::n];
    proj_fwd_wg<T, NCB, TWO>(a, (int)blockIdx.x, lds);
}
template <class T, int NDB, int NRC> __global__ __launch_bounds__(PJ_NW * 64) void k_proj_bwd_data(AumProjArgs a) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[ProjLds::n];
    proj_bwd_data_wg<T, NDB, NRC>(a, (int)blockIdx.x, lds);
}
template <class T> __global__ __launch_bounds__(PJW_NW * 64) void k_proj_bwd_weight(AumProjWArgs a, int chunk) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[ProjWLds::n];
    proj_bwd_weight_wg<T>(a, chunk, (int)blockIdx.x, lds);
}
#endif
template <class T, int NCB, bool TWO> static int proj_fwd_launch(const AumProjArgs& a, aum_stream_t s) {
    return AUM_LAUNCH((a.ntok + PJ_TT - 1) / PJ_TT, PJ_NW * 64, s, (ProjLds{}), (k_proj_fwd<T, NCB, TWO>), (proj_fwd_wg<T, NCB, TWO>(a, wg, lds)), a);
}
template <class T, int NDB, int NRC> static int proj_bwd_launch(const AumProjArgs& a, aum_stream_t s) {
    return AUM_LAUNCH((a.ntok + PJ_TT - 1) / PJ_TT, PJ_NW * 64, s, (ProjLds{}), (k_proj_bwd_data<T, NDB, NRC>), (proj_bwd_data_wg<T, NDB, NRC>(a, wg, lds)), a);
}
// shapes are compile-time in the kernels: forward (column blocks of R+2N, R > 32), backward (column blocks of R, 32-row
// k-chunks of R+2N).  R <= 64 and R+2N <= 80 bound the table.
template <class T> static int proj_t(const AumProjArgs& a, bool bwd, aum_stream_t s) {
    const int R = a.dt_rank, RT = a.dt_rank + 2 * a.dstate;
    if (!bwd) {
        const int ncb = (RT + 15) / 16;
        const bool two = R > 32;
#define AUM_PF(NCB, TWO) if (ncb == NCB && two == TWO) return proj_fwd_launch<T, NCB, TWO>(a, s);
        AUM_PF(1, false) AUM_PF(2, false) AUM_PF(3, false) AUM_PF(4, false) AUM_PF(5, false)
        AUM_PF(3, true) AUM_PF(4, true) AUM_PF(5, true)
#undef AUM_PF
        return AUM_E_UNSUPPORTED;
    }
    const int ndb = (R + 15) / 16, nrc = (RT + 31) / 32;
#define AUM_PB(NDB, NRC) if (ndb == NDB && nrc == NRC) return proj_bwd_launch<T, NDB, NRC>(a, s);
    AUM_PB(1, 1) AUM_PB(1, 2) AUM_PB(1, 3) AUM_PB(2, 1) AUM_PB(2, 2) AUM_PB(2, 3) AUM_PB(3, 2) AUM_PB(3, 3) AUM_PB(4, 2) AUM_PB(4, 3)
#undef AUM_PB
    return AUM_E_UNSUPPORTED;
}
template <class T> static int projw_t(const AumProjWArgs& a, int chunk, aum_stream_t s) {
    return AUM_LAUNCH((a.dim + PJW_ROWS - 1) / PJW_ROWS * a.nsplit, PJW_NW * 64, s, (ProjWLds{}), (k_proj_bwd_weight<T>),
                      (proj_bwd_weight_wg<T>(a, chunk, wg, lds)), a, chunk);
}
#if AUM_HAS_DTYPE(1)
int proj_bf16(const AumProjArgs& a, bool bwd, aum_stream_t s) { return proj_t<bf16_t>(a, bwd, s); }
int projw_bf16(const AumProjWArgs& a, int chunk, aum_stream_t s) { return projw_t<bf16_t>(a, chunk, s); }
#endif
#if AUM_HAS_DTYPE(2)
int proj_f16(const AumProjArgs& a, bool bwd, aum_stream_t s) { return proj_t<f16_t>(a, bwd, s); }
int projw_f16(const AumProjWArgs& a, int chunk, aum_stream_t s) { return projw_t<f16_t>(a, chunk, s); }
#endif
#endif

}  // namespace aum

// ================================================================================================
// extern "C" surface (AUM_API_PART 3 or 0): everything that is not a scan-kernel instantiation.
// ================================================================================================
#if AUM_API_PART == 3 || AUM_API_PART == 0
using namespace aum;
#define AUM_API extern "C"

AUM_API int aum_abi_version(void) { return AUM_ABI_VERSION; }
AUM_API int aum_scan_max_single_pass_len(void) { return WAVE * SCANWG_MAX_K; }   // 576 (513 uses the <8,1> geometry)

static bool scan_use_wg(int dstate, uint32_t flags) { return dstate <= SCANWG_MAX_N && !(flags & AUM_SCAN_GENERIC); }

#ifndef AUM_EMU
__global__ void k_scan_reduce(ScanReduceArgs a) {
    const ScanReduceSeg sg = a.seg[blockIdx.y];
    const bool vec = (sg.inner & 3) == 0 && ((((uintptr_t)sg.src) | ((uintptr_t)sg.dst)) & 15) == 0;
    if (vec && sg.outer >= 32 && (sg.inner >> 2) * 8 <= (int64_t)gridDim.x * blockDim.x) {
        // many partials of a short vector (dA / dD / ddelta_bias: one partial per batch entry): 32 float4 columns x 8 row groups per
        // workgroup so that the rows are read in parallel; the row groups meet in LDS in a fixed order
        __shared__ float4 part[256];
        const int64_t n4 = sg.inner >> 2;
        const float4* src = reinterpret_cast<const float4*>(sg.src);
        float4* dst = reinterpret_cast<float4*>(sg.dst);
        const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
        for (int64_t i0 = (int64_t)blockIdx.x * 32; i0 < n4; i0 += (int64_t)gridDim.x * 32) {
            const int64_t i = i0 + c;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < n4) {
                int o = rg;
                for (; o + 24 < sg.outer; o += 32) {
                    const float4 v0 = src[(int64_t)o * n4 + i], v1 = src[(int64_t)(o + 8) * n4 + i];
                    const float4 v2 = src[(int64_t)(o + 16) * n4 + i], v3 = src[(int64_t)(o + 24) * n4 + i];
                    acc.x += (v0.x + v1.x) + (v2.x + v3.x);
                    acc.y += (v0.y + v1.y) + (v2.y + v3.y);
                    acc.z += (v0.z + v1.z) + (v2.z + v3.z);
                    acc.w += (v0.w + v1.w) + (v2.w + v3.w);
                }
                for (; o < sg.outer; o += 8) {
                    const float4 v = src[(int64_t)o * n4 + i];
                    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
                }
            }
            part[threadIdx.x] = acc;
            __syncthreads();
            if (rg == 0 && i < n4) {
                float4 t = dst[i];
                for (int r = 0; r < 8; ++r) {
                    const float4 v = part[r * 32 + c];
                    t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
                }
                dst[i] = t;
            }
            __syncthreads();
        }
        return;
    }
    if (vec) {      // 16-byte accesses, four partials in flight per thread
        const int64_t n4 = sg.inner >> 2;
        const float4* src = reinterpret_cast<const float4*>(sg.src);
        float4* dst = reinterpret_cast<float4*>(sg.dst);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
            float4 acc = dst[i];
            int o = 0;
            for (; o + 4 <= sg.outer; o += 4) {
                const float4 v0 = src[(int64_t)o * n4 + i], v1 = src[(int64_t)(o + 1) * n4 + i];
                const float4 v2 = src[(int64_t)(o + 2) * n4 + i], v3 = src[(int64_t)(o + 3) * n4 + i];
                acc.x += (v0.x + v1.x) + (v2.x + v3.x);
                acc.y += (v0.y + v1.y) + (v2.y + v3.y);
                acc.z += (v0.z + v1.z) + (v2.z + v3.z);
                acc.w += (v0.w + v1.w) + (v2.w + v3.w);
            }
            for (; o < sg.outer; ++o) {
                const float4 v = src[(int64_t)o * n4 + i];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            dst[i] = acc;
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < sg.inner; i += (int64_t)gridDim.x * blockDim.x) {
        float acc = 0.f;
        for (int o = 0; o < sg.outer; ++o) acc += sg.src[(int64_t)o * sg.inner + i];
        sg.dst[i] += acc;
    }
}
#endif
#ifdef AUM_EMU
static void scan_reduce_host(const ScanReduceArgs& a) {       // what k_scan_reduce computes, as one plain loop
    for (int k = 0; k < a.nseg; ++k)
        for (int64_t i = 0; i < a.seg[k].inner; ++i) {
            float acc = 0.f;
            for (int o = 0; o < a.seg[k].outer; ++o) acc += a.seg[k].src[(int64_t)o * a.seg[k].inner + i];
            a.seg[k].dst[i] += acc;
        }
}
#endif
static int scan_reduce_launch(const ScanReduceArgs& a, aum_stream_t s) {
    return AUM_LAUNCH((Grid2{512, (unsigned)a.nseg}), 256, s, (NoLds{}), k_scan_reduce, (AUM_HOST_LOOP(scan_reduce_host(a))), a);
}

AUM_API int64_t aum_selective_scan_ckpt_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate) {
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0 || !scanwg_ct_selected(len, dstate, 0, 0u)) return 0;
    return (int64_t)batch * dim * (len / 512) * dstate * (int64_t)sizeof(float);
}

AUM_API int64_t aum_selective_scan_lane_ckpt_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional) {
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0 || !scanr_selected(len, dstate, 0u)) return 0;
    return scanr_ckpt_floats(batch, dim, dstate, bidirectional != 0) * (int64_t)sizeof(float);
}

AUM_API int64_t aum_selective_scan_workspace_bytes(int32_t batch, int32_t dim, int32_t len, int32_t dstate, int32_t bidirectional,
                                           int32_t backward) {
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0) return 0;
    if (backward && dstate <= SCANWG_MAX_N) {   // sized for the workgroup kernels (>= what the generic ones need)
        const ScanPlan wp = scanwg_plan(len);
        const ScanWgWs L = scanwg_ws_layout(batch, dim, len, dstate, scanwg_rows(batch, dim), wp.nchunks, bidirectional != 0);
        int64_t need = L.total * (int64_t)sizeof(float);
        if (scanh_selected(wp.K, wp.tail, wp.nchunks, len, dstate, 0u)) {      // the one-row kernel groups rows differently
            const int64_t h = scanwg_ws_layout(batch, dim, len, dstate, scanh_rows_for(batch, dim, bidirectional ? 2 : 0), 1, bidirectional != 0).total * (int64_t)sizeof(float);
            if (h > need) need = h;
        }
        if (scanr_selected(len, dstate, 0u)) {                                 // kernels with the lane-entry checkpoint
            const int64_t h = scanwg_ws_layout(batch, dim, len, dstate, scanr_bwd_rows(bidirectional ? 2 : 0), 1, bidirectional != 0).total * (int64_t)sizeof(float);
            if (h > need) need = h;
        }
        if (scanh_chunked_selected(len, dstate, 0, 0u)) {                      // chunked one-row kernel: 64 rows, 512-step chunks
            const int groupings[2] = {scanh_chunked_rows(batch, dim), SCANH_CH_ROWS};    // the one the launch picks; the tests' forced one
            for (int rows : groupings) {
                const int64_t h = scanwg_ws_layout(batch, dim, len, dstate, rows, len / 512, false).total * (int64_t)sizeof(float);
                if (h > need) need = h;
            }
        }
        const ScanPlan gp = scan_plan(len);
        if (gp.nchunks > 1) {
            const int64_t g = (int64_t)batch * ((dim + SCAN_R - 1) / SCAN_R) * SCAN_R * gp.nchunks * dstate * (int64_t)sizeof(float);
            if (g > need) need = g;
        }
        return need;
    }
    const ScanPlan plan = scan_plan(len);
    if (!backward || plan.nchunks == 1) return 0;
    const int64_t grid = (int64_t)batch * ((dim + SCAN_R - 1) / SCAN_R);
    return grid * SCAN_R * plan.nchunks * dstate * (int64_t)sizeof(float);
}

static int scan_common_check(const void* u, const void* delta, const void* B, const void* C, const float* A, int batch,
                             int dim, int len, int dstate, int dtype) {
    if (!u || !delta || !B || !C || !A) return AUM_E_NULL;
    if (batch <= 0 || dim <= 0 || len <= 0 || dstate <= 0) return AUM_E_SHAPE;
    if (dstate > SCAN_MAX_DSTATE) return AUM_E_UNSUPPORTED;
    if (dtype < 0 || dtype > 2) return AUM_E_DTYPE;
    return AUM_OK;
}

AUM_API int aum_selective_scan_fwd(const AumScanFwdArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    int rc = scan_common_check(a->u, a->delta, a->B, a->C, a->A, a->batch, a->dim, a->len, a->dstate, a->dtype);
    if (rc) return rc;
    if (!a->out) return AUM_E_NULL;
    const bool wgk = scan_use_wg(a->dstate, a->flags);
    ScanPlan plan = wgk ? scanwg_plan(a->len) : scan_plan(a->len);
    const bool bidir = a->A_b != nullptr;
    if (bidir && (plan.nchunks > 1 || (a->flags & AUM_SCAN_REVERSE) || a->last_state)) return AUM_E_UNSUPPORTED;
    const int mode = bidir ? 2 : ((a->flags & AUM_SCAN_REVERSE) ? 1 : 0);
    int grid = wgk ? -scanwg_rows(a->batch, a->dim) : a->batch * ((a->dim + SCAN_R - 1) / SCAN_R);
    const bool ct = wgk && scanwg_ct_selected(a->len, a->dstate, mode, a->flags);
    if (ct) {
        plan = ScanPlan{8, a->len / 512, 1};
        grid = -scanwg_ct_rows(a->batch, a->dim);
    }
    if ((a->x_ck || (a->flags & AUM_SCAN_ACCUMULATE)) && !ct) return AUM_E_UNSUPPORTED;
    const bool rowk = wgk && scanr_selected(a->len, a->dstate, a->flags);
    if (a->x_lane && !rowk) return AUM_E_UNSUPPORTED;
    if (rowk) {
        plan = ScanPlan{8, 1, SCANR_PLAN_TAIL};
        grid = -scanr_fwd_rows_for(a->batch, a->dim);
    }
    aum_stream_t s = (aum_stream_t)stream;
    return AUM_BY_DTYPE_X(a->dtype, scan_fwd, *a, plan, mode, grid, s);
}

AUM_API int aum_selective_scan_bwd(const AumScanBwdArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    int rc = scan_common_check(a->u, a->delta, a->B, a->C, a->A, a->batch, a->dim, a->len, a->dstate, a->dtype);
    if (rc) return rc;
    if (!a->dout || !a->du || !a->ddelta || !a->dA || !a->dB || !a->dC) return AUM_E_NULL;
    if (a->z && (!a->out_pre || !a->dz)) return AUM_E_NULL;
    const bool bidir = a->A_b != nullptr;
    if (bidir && !a->dA_b) return AUM_E_NULL;
    // the workgroup kernels need dense (batch, dstate, len) dB/dC (the partial-sum reduce writes them linearly)
    const bool dense = a->dB_ns == a->len && a->dC_ns == a->len && a->dB_bs == (int64_t)a->dstate * a->len &&
                       a->dC_bs == (int64_t)a->dstate * a->len;
    const bool wgk = scan_use_wg(a->dstate, a->flags) && dense;
    ScanPlan plan = wgk ? scanwg_plan(a->len) : scan_plan(a->len);
    if (bidir && (plan.nchunks > 1 || (a->flags & AUM_SCAN_REVERSE))) return AUM_E_UNSUPPORTED;
    const int mode = bidir ? 2 : ((a->flags & AUM_SCAN_REVERSE) ? 1 : 0);
    const bool chunked_rows = wgk && scanh_chunked_selected(a->len, a->dstate, mode, a->flags);
    if (chunked_rows) plan = ScanPlan{8, a->len / 512, a->len & 511};
    if (a->x_ck && !(chunked_rows && scanwg_ct_selected(a->len, a->dstate, mode, a->flags))) return AUM_E_UNSUPPORTED;
    if ((a->flags & AUM_SCAN_ACCUMULATE) && !chunked_rows) return AUM_E_UNSUPPORTED;
    const bool rowk = wgk && scanr_selected(a->len, a->dstate, a->flags);
    if (a->x_lane && !rowk) return AUM_E_UNSUPPORTED;
    const bool rowk_ck = rowk && a->x_lane;       // without the checkpoint: the previous-generation kernels recompute the states
    if (rowk_ck) plan = ScanPlan{8, 1, SCANR_PLAN_TAIL};
    aum_stream_t s = (aum_stream_t)stream;
    int rows = 0;
    int grid = a->batch * ((a->dim + SCAN_R - 1) / SCAN_R);
    if (wgk) {
        rows = rowk_ck ? scanr_bwd_rows(mode)
               : chunked_rows ? ((a->flags & AUM_DBG_CHUNKED_MAX_ROWS) ? SCANH_CH_ROWS : scanh_chunked_rows(a->batch, a->dim))
                            : scanh_selected(plan.K, plan.tail, plan.nchunks, a->len, a->dstate, a->flags) ? scanh_rows_for(a->batch, a->dim, mode) : scanwg_rows(a->batch, a->dim);
        grid = -rows;
        const ScanWgWs L = scanwg_ws_layout(a->batch, a->dim, a->len, a->dstate, rows, plan.nchunks, bidir);
        int64_t need_f = L.total;
        if (!a->workspace || a->workspace_bytes < need_f * (int64_t)sizeof(float)) return AUM_E_WORKSPACE;
    } else if (plan.nchunks > 1) {
        const int64_t need = (int64_t)grid * SCAN_R * plan.nchunks * a->dstate * (int64_t)sizeof(float);
        if (!a->workspace || a->workspace_bytes < need) return AUM_E_WORKSPACE;
    }
    const int rc2 = AUM_BY_DTYPE_X(a->dtype, scan_bwd, *a, plan, mode, grid, s);
    if (rc2 != AUM_OK || !wgk) return rc2;
    // second stage: sum the per-workgroup / per-batch partials into the (accumulate-into) outputs
    const ScanWgWs L = scanwg_ws_layout(a->batch, a->dim, a->len, a->dstate, rows, plan.nchunks, bidir);
    float* ws = (float*)a->workspace;
    ScanReduceArgs r;
    int k = 0;
    const int64_t bnl = (int64_t)a->batch * a->dstate * a->len;
    r.seg[k++] = {a->dB, ws + L.pB, bnl, L.gpb, 0};
    r.seg[k++] = {a->dC, ws + L.pC, bnl, L.gpb, 0};
    r.seg[k++] = {a->dA, ws + L.pA, (int64_t)a->dim * a->dstate, a->batch, 0};
    if (bidir) r.seg[k++] = {a->dA_b, ws + L.pAb, (int64_t)a->dim * a->dstate, a->batch, 0};
    if (a->D && a->dD) r.seg[k++] = {a->dD, ws + L.pD, (int64_t)a->dim, a->batch, 0};
    if (a->ddelta_bias) r.seg[k++] = {a->ddelta_bias, ws + L.pbias, (int64_t)a->dim, a->batch, 0};
    r.nseg = k;
    return scan_reduce_launch(r, s);
}

// ---- conv -----------------------------------------------------------------------------------
// the AuM row shape (512 + up to 8 tail steps, 16-bit activations): several rows of one channel per wave, one pass per row
template <class T, bool REV> static int conv4_rows_launch(const AumConvArgs& a, bool bwd, aum_stream_t s) {
    const int grid = a.dim * ((a.batch + CONVR_ROWS - 1) / CONVR_ROWS);
    if (bwd) return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_conv4_rows_bwd<T, REV>), (conv4_rows_bwd_wave<T, REV>(a, wg)), a);
    return AUM_LAUNCH(grid, 64, s, (NoLds{}), (k_conv4_rows_fwd<T, REV>), (conv4_rows_fwd_wave<T, REV>(a, wg)), a);
}
template <class T, bool REV> static int conv4_launch(const AumConvArgs& a, bool bwd, aum_stream_t s) {
    if constexpr (sizeof(T) == 2) {
        if (convr_shape_ok(a.len)) return conv4_rows_launch<T, REV>(a, bwd, s);
    }
    if (bwd) return AUM_LAUNCH(a.batch * a.dim, 64, s, (NoLds{}), (k_conv4_bwd<T, REV>), (conv4_bwd_wave<T, REV>(a, wg)), a);
    return AUM_LAUNCH(a.batch * a.dim, 64, s, (NoLds{}), (k_conv4_fwd<T, REV>), (conv4_fwd_wave<T, REV>(a, wg)), a);
}
template <class T> static int conv_launch(const AumConvArgs& a, bool bwd, aum_stream_t s) {
    if (a.width == 4 && !(a.flags & AUM_CONV_GENERIC))
        return with_bool((a.flags & AUM_CONV_REVERSE) != 0, [&](auto rev) { return conv4_launch<T, rev>(a, bwd, s); });
    if (bwd) return AUM_LAUNCH(a.batch * a.dim, 64, s, (ConvLds{}), (k_conv_bwd<T>), (conv_bwd_wave<T>(a, wg, lds)), a);
    return AUM_LAUNCH(a.batch * a.dim, 64, s, (NoLds{}), (k_conv_fwd<T>), (conv_fwd_wave<T>(a, wg)), a);
}
static int conv_check(const AumConvArgs* a, bool bwd) {
    if (!a || !a->x || !a->weight) return AUM_E_NULL;
    if (bwd ? (!a->dy || !a->dx || !a->dweight) : !a->y) return AUM_E_NULL;
    if (a->batch <= 0 || a->dim <= 0 || a->len <= 0 || a->width <= 0) return AUM_E_SHAPE;
    if (a->width > CONV_MAX_W) return AUM_E_UNSUPPORTED;
    if (a->dtype < 0 || a->dtype > 2) return AUM_E_DTYPE;
    return AUM_OK;
}
static int conv_dispatch(const AumConvArgs* a, bool bwd, void* stream) {
    int rc = conv_check(a, bwd);
    if (rc) return rc;
    return AUM_BY_DTYPE_T(a->dtype, conv_launch, *a, bwd, (aum_stream_t)stream);
}
AUM_API int aum_causal_conv1d_fwd(const AumConvArgs* a, void* stream) { return conv_dispatch(a, false, stream); }
AUM_API int aum_causal_conv1d_bwd(const AumConvArgs* a, void* stream) { return conv_dispatch(a, true, stream); }

// ---- rmsnorm --------------------------------------------------------------------------------
#ifndef AUM_NORM_PARTIALS
#define AUM_NORM_PARTIALS 4096      // micro-benchmark (warm caches, incl. the partial sum): 1024 / 2048 / 4096 partials = 0.145 / 0.104 / 0.108 ms, but inside the step 2048 ran 82 vs 73 us (fewer waves in flight against cold HBM)
#endif
AUM_API int aum_rmsnorm_bwd_partials(int32_t rows) { return rows < 1 ? 1 : (rows < AUM_NORM_PARTIALS ? rows : AUM_NORM_PARTIALS); }
static bool norm_is_vec(int32_t cols, uint32_t flags) { return cols <= 2048 && !(flags & AUM_NORM_GENERIC); }
// rows of dweight_partial that hold sums after aum_rmsnorm_bwd: the vectorised kernels (cols <= 2048) add NORM_BWD_NW waves' sums in the workgroup
AUM_API int aum_rmsnorm_bwd_partial_rows(int32_t rows, int32_t cols, uint32_t flags) {
    const int np = aum_rmsnorm_bwd_partials(rows);
    return norm_is_vec(cols, flags) ? (np + NORM_BWD_NW - 1) / NORM_BWD_NW : np;
}

// S: NoRowScale (aum_rmsnorm_fwd / _bwd) or RowScale (aum_rmsnorm_drop_fwd / _bwd): the same routines, grids and partial rows
template <class TX, class TR, int NCH, class S> static int norm_vec_launch(const AumNormArgs& a, bool bwd, aum_stream_t s, const S& sc) {
    const int np = aum_rmsnorm_bwd_partials(a.rows);
    if constexpr (S::on) {
        if (bwd) return AUM_LAUNCH((np + NORM_BWD_NW - 1) / NORM_BWD_NW, NORM_BWD_NW * 64, s, (NormBwdVecLds<NCH>{}), (k_norm_drop_bwd_vec<TX, TR, NCH>),
                                   (rmsnorm_bwd_vec<TX, TR, NCH>(a, wg, np, lds, sc)), a, np, sc);
        return AUM_LAUNCH(a.rows, 64, s, (NoLds{}), (k_norm_drop_fwd_vec<TX, TR, NCH>), (rmsnorm_fwd_vec<TX, TR, NCH>(a, wg, sc)), a, sc);
    } else {
        if (bwd) return AUM_LAUNCH((np + NORM_BWD_NW - 1) / NORM_BWD_NW, NORM_BWD_NW * 64, s, (NormBwdVecLds<NCH>{}), (k_norm_bwd_vec<TX, TR, NCH>),
                                   (rmsnorm_bwd_vec<TX, TR, NCH>(a, wg, np, lds)), a, np);
        return AUM_LAUNCH(a.rows, 64, s, (NoLds{}), (k_norm_fwd_vec<TX, TR, NCH>), (rmsnorm_fwd_vec<TX, TR, NCH>(a, wg)), a);
    }
}
template <class TX, class TR, class S> static int norm_launch(const AumNormArgs& a, bool bwd, aum_stream_t s, const S& sc) {
    if (norm_is_vec(a.cols, a.flags)) {
        const int nch = (a.cols + 511) / 512;
        return with_int<1, 2, 3, 4>(nch < 4 ? nch : 4, [&](auto n) { return norm_vec_launch<TX, TR, n>(a, bwd, s, sc); });
    }
    const int np = aum_rmsnorm_bwd_partials(a.rows);
    const DynLds row = {((a.cols + WAVE - 1) / WAVE) * WAVE};
    if constexpr (S::on) {
        if (bwd) return AUM_LAUNCH(np, 64, s, (row), (k_norm_drop_bwd<TX, TR>), (rmsnorm_bwd_wave<TX, TR>(a, wg, np, lds, sc)), a, np, sc);
        return AUM_LAUNCH(a.rows, 64, s, (NoLds{}), (k_norm_drop_fwd<TX, TR>), (rmsnorm_fwd_wave<TX, TR>(a, wg, sc)), a, sc);
    } else {
        if (bwd) return AUM_LAUNCH(np, 64, s, (row), (k_norm_bwd<TX, TR>), (rmsnorm_bwd_wave<TX, TR>(a, wg, np, lds)), a, np);
        return AUM_LAUNCH(a.rows, 64, s, (NoLds{}), (k_norm_fwd<TX, TR>), (rmsnorm_fwd_wave<TX, TR>(a, wg)), a);
    }
}
template <class S> static int norm_dispatch(const AumNormArgs* a, bool bwd, void* stream, const S& sc) {
    if (!a || !a->x || !a->weight) return AUM_E_NULL;
    if (bwd ? (!a->dy || !a->dx || !a->rstd_in || !a->dweight_partial) : !a->y) return AUM_E_NULL;
    if (a->rows <= 0 || a->cols <= 0) return AUM_E_SHAPE;
    if (a->cols > 16384) return AUM_E_UNSUPPORTED;
    if (a->x_dtype < 0 || a->x_dtype > 2 || a->res_dtype < 0 || a->res_dtype > 2) return AUM_E_DTYPE;
    if (a->y_dtype != a->x_dtype) return AUM_E_DTYPE;
    aum_stream_t s = (aum_stream_t)stream;
    // residual stream is fp32 (residual_in_fp32) or shares the activation dtype
    if (a->res_dtype == AUM_F32) {
        return by_dtype(a->x_dtype, norm_launch<float, float, S>, norm_launch<bf16_t, float, S>, norm_launch<f16_t, float, S>, *a, bwd, s, sc);
    }
    if (a->res_dtype != a->x_dtype) return AUM_E_DTYPE;
    if (a->x_dtype == AUM_BF16) return norm_launch<bf16_t, bf16_t>(*a, bwd, s, sc);
    return norm_launch<f16_t, f16_t>(*a, bwd, s, sc);
}
AUM_API int aum_rmsnorm_fwd(const AumNormArgs* a, void* stream) { return norm_dispatch(a, false, stream, NoRowScale{}); }
AUM_API int aum_rmsnorm_bwd(const AumNormArgs* a, void* stream) { return norm_dispatch(a, true, stream, NoRowScale{}); }

// stochastic depth: the pair above with a per-sample factor on x.  The operands the scaled routines assume are checked here, every other
// rule is norm_dispatch's.
static int norm_drop_dispatch(const AumNormDropArgs* d, bool bwd, void* stream) {
    if (!d || !d->row_scale) return AUM_E_NULL;
    const AumNormArgs* a = &d->base;
    if (bwd ? !a->dresidual_in : (!a->residual || !a->residual_out)) return AUM_E_NULL;
    if (d->rows_per_scale < 1 || a->rows % d->rows_per_scale != 0) return AUM_E_SHAPE;
    if (d->reserved != 0) return AUM_E_UNSUPPORTED;
    return norm_dispatch(a, bwd, stream, RowScale{d->row_scale, d->rows_per_scale});
}
AUM_API int aum_rmsnorm_drop_fwd(const AumNormDropArgs* a, void* stream) { return norm_drop_dispatch(a, false, stream); }
AUM_API int aum_rmsnorm_drop_bwd(const AumNormDropArgs* a, void* stream) { return norm_drop_dispatch(a, true, stream); }

// add + RMSNorm + mean over a sample's rows: the vectorised row routines of the pair above on 16-bit x and an fp32 residual stream.
// Forward: one workgroup per 32-row chunk of a sample, and where a sample has several chunks one more launch that adds them (fixed orders
// throughout, conv_norm_kernels.h).  Backward: rmsnorm_bwd_vec with its dy formed from dpooled: the grid and partial rows of aum_rmsnorm_bwd.
static_assert(NORM_POOL_CHUNK == NORM_POOL_ROWS * NORM_BWD_NW, "a chunk is the rows of one workgroup");
AUM_API int aum_rmsnorm_pool_partial_rows(int32_t rows_per_sample) { return rows_per_sample < 1 ? 0 : norm_pool_chunks(rows_per_sample); }
template <class TX> static int norm_pool_launch(const AumNormPoolArgs& q, bool bwd, aum_stream_t s) {
    const AumNormArgs& a = q.base;
    const int nch = (a.cols + 511) / 512;
    if (bwd) {
        const int np = aum_rmsnorm_bwd_partials(a.rows);
        const DyPooled g = {q.dpooled, q.row_stride_dpooled, q.rows_per_sample};
        return with_int<1, 2, 3, 4>(nch, [&](auto n) {
            constexpr int N = decltype(n)::value;
            return AUM_LAUNCH((np + NORM_BWD_NW - 1) / NORM_BWD_NW, NORM_BWD_NW * 64, s, (NormBwdVecLds<N>{}), (k_norm_pool_bwd_vec<TX, N>),
                              (rmsnorm_bwd_vec<TX, float, N, NoRowScale, DyPooled>(a, wg, np, lds, NoRowScale{}, g)), a, np, g);
        });
    }
    const int samples = a.rows / q.rows_per_sample, nchunk = norm_pool_chunks(q.rows_per_sample);
    const int rc = with_int<1, 2, 3, 4>(nch, [&](auto n) {
        constexpr int N = decltype(n)::value;
        return AUM_LAUNCH((int64_t)samples * nchunk, NORM_BWD_NW * 64, s, (NormBwdVecLds<N>{}), (k_norm_pool_fwd_vec<TX, N>),
                          (rmsnorm_pool_fwd_vec<TX, float, N>(q, wg, lds)), q);
    });
    if (rc || nchunk == 1) return rc;
    return AUM_LAUNCH((int64_t)samples * nch, 64, s, (NoLds{}), (k_norm_pool_finish<TX>), (rmsnorm_pool_finish<TX>(q, wg)), q);
}
static int norm_pool_dispatch(const AumNormPoolArgs* q, bool bwd, void* stream) {
    if (!q) return AUM_E_NULL;
    const AumNormArgs* a = &q->base;
    if (!a->x || !a->weight) return AUM_E_NULL;
    if (bwd ? (!q->dpooled || !a->rstd_in || !a->dx || !a->dresidual_in || !a->dweight_partial) : (!a->residual || !q->pooled)) return AUM_E_NULL;
    if (a->rows <= 0 || a->cols <= 0 || q->rows_per_sample < 1 || a->rows % q->rows_per_sample != 0) return AUM_E_SHAPE;
    if (a->x_dtype < 0 || a->x_dtype > 2 || a->res_dtype < 0 || a->res_dtype > 2 || a->y_dtype != a->x_dtype) return AUM_E_DTYPE;
    if (a->x_dtype == AUM_F32 || a->res_dtype != AUM_F32 || a->flags != 0 || q->reserved != 0) return AUM_E_UNSUPPORTED;
    if (a->cols % 8 != 0 || a->cols > 2048) return AUM_E_UNSUPPORTED;
    if (a->y || a->dy || a->dresidual_out) return AUM_E_UNSUPPORTED;
    if (!bwd) {
        if ((a->residual_out == nullptr) != (a->rstd_out == nullptr)) return AUM_E_UNSUPPORTED;
        if (norm_pool_chunks(q->rows_per_sample) > 1 && !q->pool_partial) return AUM_E_NULL;
        if ((int64_t)(a->rows / q->rows_per_sample) * norm_pool_chunks(q->rows_per_sample) > 0x7fffffff) return AUM_E_SHAPE;
    }
    aum_stream_t s = (aum_stream_t)stream;
    return a->x_dtype == AUM_BF16 ? norm_pool_launch<bf16_t>(*q, bwd, s) : norm_pool_launch<f16_t>(*q, bwd, s);
}
AUM_API int aum_rmsnorm_pool_fwd(const AumNormPoolArgs* a, void* stream) { return norm_pool_dispatch(a, false, stream); }
AUM_API int aum_rmsnorm_pool_bwd(const AumNormPoolArgs* a, void* stream) { return norm_pool_dispatch(a, true, stream); }

// ---- fbank frontend ----------------------------------------------------------------------------
typedef Lds<float, FBANK_LDS_FLOATS> FbankLds;
typedef Lds<float, FBANK_NW * FBW_WAVE_FLOATS> FbankWLds;
#ifndef AUM_EMU
__global__ __launch_bounds__(FBANK_THREADS) void k_fbank(AumFbankArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[FbankLds::n];
    fbank_frame(a, (int)blockIdx.x, lds);
}
__global__ __launch_bounds__(FBANK_THREADS) void k_fbank_w(AumFbankArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[FbankWLds::n];
    fbank_frames_wg(a, (int)blockIdx.x, lds);
}
#endif
AUM_API int aum_fbank_fwd(const AumFbankArgs* a, void* stream) {
    if (!a || !a->wave || !a->out || !a->window || !a->twiddle || !a->mel_start_f || !a->mel_count_f || !a->mel_w) return AUM_E_NULL;
    if (a->batch <= 0 || a->win <= 0 || a->shift <= 0 || a->num_mel <= 0 || a->target_length <= 0) return AUM_E_SHAPE;
    if (a->padded < a->win || a->padded > FBANK_MAX_FFT || (a->padded & (a->padded - 1)) || a->padded < 2 * WAVE) return AUM_E_UNSUPPORTED;
    if (a->num_frames < 0 || (a->num_frames > 0 && (int64_t)(a->num_frames - 1) * a->shift + a->win > a->n_samples)) return AUM_E_SHAPE;
    const int grid = a->batch * a->target_length;
    const bool per_wave = a->padded == FBW_N;      // the 16 kHz / 25 ms configuration: one wavefront per frame
    aum_stream_t s = (aum_stream_t)stream;
    if (per_wave) return AUM_LAUNCH((grid + FBW_WG_FRAMES - 1) / FBW_WG_FRAMES, FBANK_THREADS, s, (FbankWLds{}), k_fbank_w, (fbank_frames_wg(*a, wg, lds)), *a);
    return AUM_LAUNCH(grid, FBANK_THREADS, s, (FbankLds{}), k_fbank, (fbank_frame(*a, wg, lds)), *a);
}

// ---- EPIC-Sounds frontend: log-mel (librosa-style STFT) and the SpecAugment time warp ------------------------------
typedef Lds<float, STFT_LDS_FLOATS> StftLds;
#ifndef AUM_EMU
__global__ __launch_bounds__(STFT_THREADS) void k_stft_logmel(AumStftArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[StftLds::n];
    stft_logmel_frame(a, (int)blockIdx.x, lds);
}
__global__ __launch_bounds__(STFT_THREADS) void k_spec_time_warp(AumTimeWarpArgs a) { spec_time_warp_wg(a, (int)blockIdx.x); }
#endif
AUM_API int aum_stft_logmel_fwd(const AumStftArgs* a, void* stream) {
    if (!a || !a->wave || !a->n_valid || !a->out || !a->window || !a->twiddle || !a->mel_start_f || !a->mel_count_f || !a->mel_w) return AUM_E_NULL;
    if (a->batch <= 0 || a->n_samples < 0 || a->win <= 0 || a->hop <= 0 || a->num_mel <= 0 || a->mel_wstride <= 0 || a->target_length <= 0)
        return AUM_E_SHAPE;
    if (a->n_fft < 256 || a->n_fft > AUM_STFT_MAX_FFT || (a->n_fft & (a->n_fft - 1)) || a->win > a->n_fft) return AUM_E_UNSUPPORTED;
    if ((int64_t)a->batch * a->target_length > 0x7fffffff) return AUM_E_SHAPE;
    return AUM_LAUNCH(a->batch * a->target_length, STFT_THREADS, (aum_stream_t)stream, (StftLds{}), k_stft_logmel, (stft_logmel_frame(*a, wg, lds)), *a);
}
AUM_API int aum_spec_time_warp(const AumTimeWarpArgs* a, void* stream) {
    if (!a || !a->in || !a->table || !a->out) return AUM_E_NULL;
    if (a->in == a->out) return AUM_E_UNSUPPORTED;
    if (a->batch <= 0 || a->frames < 2 || a->num_mel < 2 || (int64_t)a->frames * a->num_mel < WAVE) return AUM_E_SHAPE;
    const int64_t per_clip = (int64_t)a->frames * a->num_mel;
    if (per_clip + WAVE > 0x7fffffff || a->in_bs < per_clip || a->out_bs < per_clip) return AUM_E_SHAPE;
    const int64_t grid = (per_clip * a->batch + STFT_THREADS - 1) / STFT_THREADS;
    if (grid > 0x7fffffff) return AUM_E_SHAPE;
    return AUM_LAUNCH(grid, STFT_THREADS, (aum_stream_t)stream, (NoLds{}), k_spec_time_warp, (spec_time_warp_wg(*a, wg)), *a);
}

// ---- waveform -> tokens in one launch ------------------------------------------------------------
typedef Lds<float, FT_LDS_FLOATS> FrontendLds;
typedef Lds<uint16_t, FT_TILE> FrontendTile;
#ifndef AUM_EMU
template <class T, class TO> __global__ __launch_bounds__(FT_NW * 64, 4) void k_frontend_tokens(AumFrontendArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[FrontendLds::n];
    __shared__ __attribute__((aligned(16))) uint16_t tile[FrontendTile::n];
    frontend_tokens_wg<T, TO>(a, (int)blockIdx.x, lds, tile);
}
#endif
template <class T, class TO> static int frontend_launch(const AumFrontendArgs& a, aum_stream_t s) {
    return AUM_LAUNCH(a.fbank.batch * (a.fbank.target_length / FT_FRAMES), FT_NW * 64, s, (FrontendLds{}, FrontendTile{}), (k_frontend_tokens<T, TO>),
                      (frontend_tokens_wg<T, TO>(a, wg, lds, lds2)), a);
}
AUM_API int aum_frontend_tokens_fwd(const AumFrontendArgs* a, void* stream) {
    if (!a) return AUM_E_NULL;
    const AumFbankArgs& f = a->fbank;
    if (!f.wave || !f.window || !f.twiddle || !f.mel_start_f || !f.mel_count_f || !f.mel_w) return AUM_E_NULL;
    if (!a->weight || !a->bias || !a->pos || !a->tokens) return AUM_E_NULL;
    if (f.batch <= 0 || f.win <= 0 || f.shift <= 0 || f.target_length <= 0 || a->dim <= 0) return AUM_E_SHAPE;
    if (f.num_frames < 0 || (f.num_frames > 0 && (int64_t)(f.num_frames - 1) * f.shift + f.win > f.n_samples)) return AUM_E_SHAPE;
    if (a->dtype != AUM_BF16 && a->dtype != AUM_F16) return a->dtype == AUM_F32 ? AUM_E_UNSUPPORTED : AUM_E_DTYPE;
    if (a->out_dtype != AUM_F32 && a->out_dtype != a->dtype) return AUM_E_DTYPE;
    if (f.padded != FBW_N || f.win > FBW_N || f.num_mel != FT_MEL || f.target_length % FT_FRAMES || a->dim % 16) return AUM_E_UNSUPPORTED;
    const int64_t n_tok = (int64_t)f.target_length / 16 * (FT_MEL / 16) + (a->cls_row ? 1 : 0);
    if (a->cls_row && (a->cls_pos < 0 || a->cls_pos >= n_tok)) return AUM_E_SHAPE;
    if (a->tokens_bs < n_tok * a->dim || n_tok * a->dim >= ((int64_t)1 << 31)) return AUM_E_SHAPE;
    aum_stream_t s = (aum_stream_t)stream;
    if (a->dtype == AUM_BF16) return a->out_dtype == AUM_F32 ? frontend_launch<bf16_t, float>(*a, s) : frontend_launch<bf16_t, bf16_t>(*a, s);
    return a->out_dtype == AUM_F32 ? frontend_launch<f16_t, float>(*a, s) : frontend_launch<f16_t, f16_t>(*a, s);
}

// ---- skinny projections (MFMA): argument checks here, kernels in the AUM_API_PART 4 objects ---------------------
static int proj_check(const AumProjArgs* a, bool bwd) {
    if (!a || !a->act || !a->w_x || !a->w_dt || !a->x_dbl || !a->out_act) return AUM_E_NULL;
    if (bwd && (!a->dB || !a->dC)) return AUM_E_NULL;
    if (a->ntok <= 0 || a->dim <= 0 || a->dt_rank <= 0 || a->dstate <= 0 || (bwd && a->len <= 0)) return AUM_E_SHAPE;
    if (a->dtype != AUM_BF16 && a->dtype != AUM_F16) return a->dtype == AUM_F32 ? AUM_E_UNSUPPORTED : AUM_E_DTYPE;
    if (a->dim % 64 || a->dt_rank > 64 || a->dt_rank + 2 * a->dstate > 16 * PJ_MAXRB) return AUM_E_UNSUPPORTED;
    if (a->w_ld % 8 || a->w_ld < (bwd ? a->dt_rank + 2 * a->dstate : a->dt_rank)) return AUM_E_SHAPE;
    if (a->ntok * 80 >= ((int64_t)1 << 31) || (int64_t)a->dim * 80 >= ((int64_t)1 << 31)) return AUM_E_UNSUPPORTED;
    return AUM_OK;
}
AUM_API int aum_proj_fwd(const AumProjArgs* a, void* stream) {
    const int rc = proj_check(a, false);
    if (rc) return rc;
    return a->dtype == AUM_BF16 ? proj_bf16(*a, false, (aum_stream_t)stream) : proj_f16(*a, false, (aum_stream_t)stream);
}
AUM_API int aum_proj_bwd_data(const AumProjArgs* a, void* stream) {
    const int rc = proj_check(a, true);
    if (rc) return rc;
    return a->dtype == AUM_BF16 ? proj_bf16(*a, true, (aum_stream_t)stream) : proj_f16(*a, true, (aum_stream_t)stream);
}
AUM_API int aum_proj_bwd_weight_splits(int32_t dim, int64_t ntok) {
    if (dim <= 0 || dim % 64 || ntok <= 0) return 0;
    const int nec = (dim + PJW_ROWS - 1) / PJW_ROWS;
    // two workgroups per CU and never one more: 43 splits x 12 channel blocks = 516 workgroups left four of them to run after the
    // other 512 (cold-cache sweep, dW_x incl. the partial sum: 21/42/43/64/86/128 splits = 69/61/67/65/76/87 us)
    int64_t s = (2 * 256) / nec;
    const int64_t most = (ntok + 127) / 128;                        // at least 128 tokens per workgroup
    if (s > most) s = most;
    return (int)(s < 1 ? 1 : s);
}
AUM_API int aum_proj_bwd_weight(const AumProjWArgs* a, void* stream) {
    if (!a || !a->x || !a->y || !a->out) return AUM_E_NULL;
    if (a->ntok <= 0 || a->dim <= 0 || a->nrows <= 0 || a->nsplit <= 0) return AUM_E_SHAPE;
    if (a->dtype != AUM_BF16 && a->dtype != AUM_F16) return a->dtype == AUM_F32 ? AUM_E_UNSUPPORTED : AUM_E_DTYPE;
    if (a->dim % 64 || a->nrows > 16 * PJ_MAXRB || a->ntok * 80 >= ((int64_t)1 << 31)) return AUM_E_UNSUPPORTED;
    const int64_t per_wg = (a->ntok + a->nsplit - 1) / a->nsplit;
    const int chunk = (int)((per_wg + PJW_KS - 1) / PJW_KS * PJW_KS);
    return a->dtype == AUM_BF16 ? projw_bf16(*a, chunk, (aum_stream_t)stream) : projw_f16(*a, chunk, (aum_stream_t)stream);
}

// ---- self-test / calibration, sums and copies: kernels whose lane-array form is one plain host loop (a grid of one) -------
#ifdef AUM_EMU
static void selftest_scan_host(const float* in, float* out, int rev) {
    vf P, S;
    for (int l = 0; l < 64; ++l) { P.v[l] = in[l]; S.v[l] = in[64 + l]; }
    if (rev) wave_scan_affine<true>(P, S); else wave_scan_affine<false>(P, S);
    for (int l = 0; l < 64; ++l) { out[l] = P.v[l]; out[64 + l] = S.v[l]; }
}
static void selftest_sum32_host(const float* in, float* out) {
    vf v[32];
    for (int k = 0; k < 32; ++k)
        for (int l = 0; l < 64; ++l) v[k].v[l] = in[k * 64 + l];
    vf w[16];
    for (int k = 0; k < 16; ++k) w[k] = v[k];
    const vf r16 = wave_sum16(w);
    const vf r = wave_sum32(v);
    for (int l = 0; l < 64; ++l) { out[l] = r.v[l]; out[64 + l] = r16.v[l]; }
}
template <class T> static void sum_rows_host(const T* p, float* dst, int64_t batch, int64_t outer, int64_t inner) {
    for (int64_t b = 0; b < batch; ++b)
        for (int64_t i = 0; i < inner; ++i) {
            float acc = 0.f;
            for (int64_t o = 0; o < outer; ++o) acc += elem_to_f32(p[(b * outer + o) * inner + i]);
            dst[b * inner + i] = acc;
        }
}
static void sum_rows_multi_host(const AumSumJob* jobs, int njobs) {
    for (int q = 0; q < njobs; ++q) {
        const AumSumJob& j = jobs[q];
        for (int64_t i = 0; i < j.inner; ++i) {
            float acc = 0.f;
            for (int64_t o = 0; o < j.outer; ++o) acc += j.src[o * j.inner + i];
            j.dst[j.tr_cols > 0 ? (i % j.tr_cols) * (j.inner / j.tr_cols) + i / j.tr_cols : i] = acc;
        }
    }
}
#endif
AUM_API int aum_selftest_wave_scan(const float* in, float* out, int rev, void* stream) {
    if (!in || !out) return AUM_E_NULL;
    return AUM_LAUNCH(1, 64, (aum_stream_t)stream, (NoLds{}), k_selftest_scan, (AUM_HOST_LOOP(selftest_scan_host(in, out, rev))), in, out, rev);
}

// wave_sum32 on 32 x 64 values (in[k][lane]); out[lane] = total of value wave_sum32_value_of_lane(lane); out[64 + lane] = wave_sum16 of
// the first 16 values.  out: 2 x 64 floats
AUM_API int aum_selftest_wave_sum32(const float* in, float* out, void* stream) {
    if (!in || !out) return AUM_E_NULL;
    return AUM_LAUNCH(1, 64, (aum_stream_t)stream, (NoLds{}), k_selftest_sum32, (AUM_HOST_LOOP(selftest_sum32_host(in, out))), in, out);
}

// row groups per workgroup: enough workgroups to cover the chip when `inner` is small (norm partials: 2048 x 768), one row group
// (no LDS pass) when `inner` alone gives thousands of them (split-K partial products: 8 x 1.2 M)
static int sum_rows_rg(int64_t work, int64_t outer) {
    return (work >= 256 * 512 || outer <= 2) ? 1 : (work >= 64 * 512 || outer <= 8) ? 4 : (work >= 16 * 512 || outer <= 32) ? 16 : 64;
}

template <class T> static int sum_rows_t(const void* src, float* dst, int64_t batch, int64_t outer, int64_t inner, aum_stream_t s) {
    const int64_t cols = inner / 8;
    const T* p = static_cast<const T*>(src);
    return with_int<1, 4, 16, 64>(sum_rows_rg(cols * batch, outer), [&](auto rg) {       // column groups over all batch entries
        return AUM_LAUNCH((Grid2{(unsigned)((cols + 256 / rg - 1) / (256 / rg)), (unsigned)batch}), 256, s, (NoLds{}), (k_sum_rows<T, rg>),
                          (AUM_HOST_LOOP(sum_rows_host(p, dst, batch, outer, inner))), p, dst, outer, inner);
    });
}
AUM_API int aum_sum_rows(const void* src, float* dst, int64_t batch, int64_t outer, int64_t inner, int32_t src_dtype, void* stream) {
    if (!src || !dst) return AUM_E_NULL;
    if (batch <= 0 || batch > 65535 || outer <= 0 || inner <= 0 || (inner & 7)) return AUM_E_SHAPE;
    if ((((uintptr_t)src) & 15) || (((uintptr_t)dst) & 3)) return AUM_E_SHAPE;          // dst: any 4-byte aligned float address (a gradient's view in a bucket; aum_hip._sum_out)
    if (src_dtype < 0 || src_dtype > 2) return AUM_E_DTYPE;
    return AUM_BY_DTYPE_T(src_dtype, sum_rows_t, src, dst, batch, outer, inner, (aum_stream_t)stream);
}

AUM_API int aum_sum_rows_multi(const AumSumJob* jobs, int32_t njobs, void* stream) {
    if (!jobs) return AUM_E_NULL;
    if (njobs < 1 || njobs > AUM_SUM_MAX_JOBS) return AUM_E_SHAPE;
    for (int q = 0; q < njobs; ++q) {
        const AumSumJob& j = jobs[q];
        if (!j.src || !j.dst) return AUM_E_NULL;
        if (j.outer <= 0 || j.inner <= 0 || (j.inner & 7) || j.inner > (int64_t)1 << 30 || j.tr_cols < 0 || (j.tr_cols > 0 && j.inner % j.tr_cols)) return AUM_E_SHAPE;
        if ((((uintptr_t)j.src) & 15) || (((uintptr_t)j.dst) & 3)) return AUM_E_SHAPE;
    }
#ifdef AUM_EMU      // the kernel takes its jobs as SumJobs, a device-only struct of conv_norm_kernels.h: the two builds marshal differently
    return AUM_LAUNCH(1, 256, (aum_stream_t)stream, (NoLds{}), k_sum_rows_multi, (AUM_HOST_LOOP(sum_rows_multi_host(jobs, njobs))), jobs);
#else
    static_assert(SUM_MAX_JOBS == AUM_SUM_MAX_JOBS, "header and kernel disagree");
    SumJobs js{};
    int64_t wgs = 0;
    for (int q = 0; q < SUM_MAX_JOBS; ++q) {
        if (q < njobs) {
            const AumSumJob& j = jobs[q];
            const int rg = sum_rows_rg(j.inner / 8, j.outer);
            js.src[q] = j.src, js.dst[q] = j.dst, js.outer[q] = j.outer, js.inner[q] = j.inner, js.tr_cols[q] = j.tr_cols, js.rg[q] = rg;
            wgs += (j.inner / 8 + 256 / rg - 1) / (256 / rg);
        }
        js.wg_end[q] = (int32_t)wgs;
    }
    if (wgs > 0x7fffffff) return AUM_E_SHAPE;
    return AUM_LAUNCH(wgs, 256, (aum_stream_t)stream, (NoLds{}), k_sum_rows_multi, (0), js);
#endif
}

AUM_API int aum_hbm_copy(const void* src, void* dst, int64_t bytes, void* stream) {
    if (!src || !dst) return AUM_E_NULL;
    if (bytes <= 0 || (bytes & 15)) return AUM_E_SHAPE;
    if (bytes / 16 / 256 >= ((int64_t)1 << 31) - 1) return AUM_E_SHAPE;
    return AUM_LAUNCH((bytes / 16 + 255) / 256, 256, (aum_stream_t)stream, (NoLds{}), k_hbm_copy, (AUM_HOST_LOOP(memcpy(dst, src, (size_t)bytes))),
                      (const float4*)src, (float4*)dst, bytes / 16);
}

#endif

#include "aum_api_tm.inc"
