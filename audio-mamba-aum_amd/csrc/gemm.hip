// gemm.hip -- translation unit of the plain-HIP MFMA kernels (no wave.h): the dense projection GEMMs (gemm_kernels.h, gemm_ps_kernels.h), the
// dt and x/dt projections of the token-major block (dtproj_kernels.h, xdt_kernels.h), the single-token decode kernels and the weight-bank
// cast; include/aum_hip.h.  Every entry: argument check of its *_args.h, stream, one dispatch expression (with_bool / with_int / by_dtype of
// launch.h) that ends in launch() below.  A value that a with_int list does not hold is AUM_E_UNSUPPORTED: nothing falls into a default.
#include <atomic>
#include "gemm_kernels.h"
#include "gemm_ps_kernels.h"
#include "dtproj_kernels.h"
#include "xdt_kernels.h"
#include "decode_kernels.h"
#include "cast_kernels.h"
#include "launch.h"

using aum::with_bool;
using aum::with_int;

// THE launch of this unit (every kernel here takes one argument struct and static LDS).  It clears the HIP error first: a stale error of
// an earlier, unrelated launch must not be reported as this one's
template <class A> static int launch(void (*kernel)(A), int64_t grid, int block, hipStream_t s, const A& a) {
    (void)hipGetLastError();
    return AUM_LAUNCH(grid, block, s, (aum::NoLds{}), kernel, (0), a);
}

// CU count of the CURRENT device (one process may drive several devices from several threads): a small per-device cache, filled with
// relaxed atomics -- racing fillers write the same value
static int cu_count() {
    static std::atomic<int> ncu_of[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int ncu = ncu_of[dev].load(std::memory_order_relaxed);
    if (!ncu) {
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) return 0;
        ncu_of[dev].store(ncu, std::memory_order_relaxed);
    }
    return ncu;
}

extern "C" int aum_gemm_tn(const AumGemmArgs* p, void* stream) {
    if (const int rc = aumg::gemm_check(p)) return rc;
    const AumGemmArgs& g = *p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ncu = cu_count();
    if (ncu <= 0) return AUM_E_LAUNCH;
    // Which kernel: the paced-store kernel (round 6, gemm_ps_kernels.h: one workgroup per CU walking a tile list, a tile's stores under the
    // next tile's K-steps) whenever a tile has the seven K-steps its store pacing needs -- every projection of the model (k >= 768);
    // shorter products: one workgroup per tile, software-pipelined K loop (round 4).  AUM_GEMM_LOCKSTEP / _PIPELINED / _PACED name one.
    uint32_t flags = g.flags & (AUM_GEMM_LOCKSTEP | AUM_GEMM_PIPELINED | AUM_GEMM_PACED);
    if (!flags) flags = g.k >= (aumg::PS_NST + 1) * aumg::BK ? AUM_GEMM_PACED : AUM_GEMM_PIPELINED;
    if ((flags & AUM_GEMM_PACED) && g.k < (aumg::PS_NST + 1) * aumg::BK) return AUM_E_UNSUPPORTED;
    return with_bool(g.dtype == AUM_BF16, [&](auto bf) {
        if (flags & AUM_GEMM_PACED) {
            aumg::GemmLaunch L;
            L.g = g;
            aumg::gemm_ps_items(g.m, g.n, ncu, &L);
            return launch(aumg::k_gemm_tn_ps<bf>, L.nitems < ncu ? L.nitems : ncu, aumg::THREADS, s, L);
        }
        const int tiles = (g.m + aumg::BM - 1) / aumg::BM * (g.n / aumg::BN);
        return with_bool((flags & AUM_GEMM_PIPELINED) != 0, [&](auto piped) { return launch(aumg::k_gemm_tn<bf, piped ? 2 : 0>, tiles, aumg::THREADS, s, g); });
    });
}

extern "C" int aum_gemm_wgrad(const AumGemmWArgs* p, void* stream) {
    if (const int rc = aumg::gemm_wgrad_check(p)) return rc;
    const AumGemmWArgs& g = *p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool skinny = g.k % 256 != 0;
    const int nitems = (g.n / 256) * (skinny ? 1 : g.k / 256) * g.splits;
    const int grid = (nitems + 7) / 8 * 8;          // eight XCD runs of equal length; the surplus workgroups return at once
    return with_bool(g.dtype == AUM_BF16, [&](auto bf) {
        if (!skinny) return launch(aumg::k_gemm_wgrad<bf>, grid, aumg::THREADS, s, g);
        return with_int<WGRAD_SKINNY_K>(g.k, [&](auto k) { return launch(aumg::k_gemm_wgrad_skinny<bf, k>, grid, aumg::THREADS, s, g); });
    });
}

extern "C" int aum_dtproj_tm_fwd(const AumDtProjArgs* p, void* stream) {
    if (const int rc = aumd::dtproj_check(p)) return rc;
    const AumDtProjArgs& g = *p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t nwaves = (g.ntok + aumd::TOK_PER_WAVE - 1) / aumd::TOK_PER_WAVE;
    return with_bool(g.dtype == AUM_BF16, [&](auto bf) {
        return with_bool(g.rank <= 32, [&](auto one) {
            return launch(aumd::k_dtproj_tm<bf, one ? 1 : 2>, (nwaves + aumd::WAVES - 1) / aumd::WAVES, aumd::WAVES * 64, s, g);
        });
    });
}

// both x/dt entries: f(nw) with the waves per workgroup of `ntok` tokens on this device (xdt_waves) as a constant; the grid of nw waves
template <class F> static int with_xdt_waves(int64_t ntok, F&& f) {
    const int ncu = cu_count();
    if (ncu <= 0) return AUM_E_LAUNCH;
    return with_int<XDT_WAVES>(aumx::xdt_waves(ntok, ncu), f);
}
static int64_t xdt_grid(int64_t ntok, int nw) { return (ntok + nw * XDT_TOK_W - 1) / (nw * XDT_TOK_W); }

extern "C" int aum_xdt_tm_fwd(const AumXdtArgs* p, void* stream) {
    if (const int rc = aumx::xdt_check(p)) return rc;
    const AumXdtArgs& g = *p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_xdt_waves(g.ntok, [&](auto nw) {
        return with_int<XDT_FWD_WIDTHS>(g.ncols, [&](auto nc) {
            return with_bool((g.flags & AUM_XDT_DELTA_SOFTPLUS) != 0, [&](auto sp) {
                return with_bool(g.dtype == AUM_BF16, [&](auto bf) {
                    return with_bool(g.rank <= 32, [&](auto one) {
                        return launch(aumx::k_xdt_tm_fwd<bf, one ? 1 : 2, nw, nc, sp>, xdt_grid(g.ntok, nw), nw * 64, s, g);
                    });
                });
            });
        });
    });
}

extern "C" int aum_xdt_tm_bwd(const AumXdtBwdArgs* p, void* stream) {
    if (const int rc = aumx::xdt_bwd_check(p)) return rc;
    const AumXdtBwdArgs& g = *p;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_xdt_waves(g.ntok, [&](auto nw) {
        return with_int<XDT_BWD_WIDTHS>(g.ncols, [&](auto nc) {          // (ncols, rank): (80, 48) or (56, 24), xdt_bwd_check
            return with_bool(g.dtype == AUM_BF16, [&](auto bf) {
                // du read-ahead of four channel pairs where a quarter of the channels holds a multiple of four
                return with_bool(g.dim % 512 == 0, [&](auto deep) {
                    return launch(aumx::k_xdt_tm_bwd<bf, nc, nw, deep ? 4 : 2>, xdt_grid(g.ntok, nw), nw * 64, s, g);
                });
            });
        });
    });
}

template <class T> static int conv_update_launch(const AumConvUpdateArgs& a, int64_t grid, hipStream_t s) { return launch(aumdec::k_conv_update<T>, grid, 256, s, a); }
template <class T> static int state_update_launch(const AumStateUpdateArgs& a, int64_t grid, hipStream_t s) { return launch(aumdec::k_state_update<T>, grid, 256, s, a); }

extern "C" int aum_causal_conv1d_update(const AumConvUpdateArgs* p, void* stream) {
    if (const int rc = aumdec::conv_update_check(p)) return rc;
    const int64_t n = (int64_t)p->batch * p->dim;
    return aum::by_dtype(p->dtype, conv_update_launch<float>, conv_update_launch<__bf16>, conv_update_launch<_Float16>, *p, (n + 255) / 256,
                         static_cast<hipStream_t>(stream));
}

extern "C" int aum_selective_state_update(const AumStateUpdateArgs* p, void* stream) {
    if (const int rc = aumdec::state_update_check(p)) return rc;
    const int64_t n = (int64_t)p->batch * p->dim;
    return aum::by_dtype(p->dtype, state_update_launch<float>, state_update_launch<__bf16>, state_update_launch<_Float16>, *p, (n + 255) / 256,
                         static_cast<hipStream_t>(stream));
}

extern "C" int aum_cast_bank(const uint64_t* src, int32_t n, int32_t rows, int32_t cols, void* bank, void* bank_t, int32_t dtype, void* stream) {
    if (const int rc = aumc::cast_bank_check(src, bank, bank_t, n, rows, cols, dtype)) return rc;
    aumc::CastBank a;
    a.src = src, a.bank = bank, a.bank_t = bank_t, a.n = n, a.rows = rows, a.cols = cols;
    a.tiles_r = (rows + aumc::CT - 1) / aumc::CT, a.tiles_c = (cols + aumc::CT - 1) / aumc::CT;
    return with_bool(dtype == AUM_BF16, [&](auto bf) {
        return launch(aumc::k_cast_bank<bf>, (int64_t)a.tiles_r * a.tiles_c * n, 256, static_cast<hipStream_t>(stream), a);
    });
}
