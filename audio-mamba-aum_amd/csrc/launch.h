// launch.h -- how the host code of aum_api.inc / aum_api_tm.inc and gemm.hip starts a kernel and picks its instantiation.  Shared by the gfx950 build and
// the lane-array build (AUM_EMU), which has no kernels: there a launch is a loop of the kernel's workgroup body over the grid.
//
//   Lds<E, N>        the LDS array of a kernel, stated once: the __shared__ array of the k_* entry is E[L::n], and the lane-array build
//                    allocates the same count for a launch -- a body that reaches past it is out of bounds in both builds.
//   AUM_LAUNCH       the one launch: grid, workgroup size, stream, LDS, kernel, workgroup body, kernel arguments; ends in launch_status().
//                    It does not clear the HIP error first, so an entry of aum_api.inc / aum_api_tm.inc reports whatever error is pending.
//                    gemm.hip alone clears, in its launch() around AUM_LAUNCH: its entries have always promised that a stale error of an
//                    earlier, unrelated launch is not reported as theirs.
//   with_bool / with_int / by_dtype   runtime flags, small integers and the activation dtype into template parameters.
#pragma once
#include <type_traits>
#ifdef AUM_EMU
#include <vector>
#endif

namespace aum {

template <class E, int N> struct Lds {
    typedef E elem;
    static constexpr int n = N;
    static constexpr int count() { return N; }
};
typedef Lds<float, 0> NoLds;
struct DynLds {                   // sized per launch (extern __shared__ float[])
    typedef float elem;
    int n_floats;
    int count() const { return n_floats; }
};
template <class L> static constexpr size_t lds_dyn_bytes(const L&) { return 0; }
static inline size_t lds_dyn_bytes(const DynLds& l) { return (size_t)l.n_floats * sizeof(float); }
template <class L, class L2> static constexpr size_t lds_dyn_bytes(const L&, const L2&) { return 0; }
struct Grid2 { unsigned x, y; };  // a two-dimensional grid (blockIdx.x, blockIdx.y); every other grid is a count

#ifdef AUM_EMU
typedef void* aum_stream_t;
static int launch_status() { return AUM_OK; }
// body(wg, lds, lds2) for wg = 0 .. grid-1 on freshly allocated LDS
static inline int64_t grid_count(int64_t g) { return g; }
static inline int64_t grid_count(Grid2 g) { return (int64_t)g.x * g.y; }
template <class F, class L, class L2 = NoLds> static int emu_launch(int64_t grid, F&& body, const L& l, const L2& l2 = L2{}) {
    std::vector<typename L::elem> lds(l.count());
    std::vector<typename L2::elem> lds2(l2.count());
    for (int64_t wg = 0; wg < grid; ++wg) body((int)wg, lds.data(), lds2.data());
    return launch_status();
}
#define AUM_UNPAREN(...) __VA_ARGS__
// LDS, KERNEL and BODY in parentheses; BODY is an expression in `wg`, `lds` (and `lds2`), evaluated once per workgroup.  KERNEL and the
// kernel arguments are the device build's alone.  AUM_HOST_LOOP(call): the body of a kernel whose lane-array form is one plain host loop --
// it runs in workgroup 0, the other workgroups of the grid do nothing.
#define AUM_HOST_LOOP(...) (wg == 0 ? (void)(__VA_ARGS__) : (void)0)
#define AUM_LAUNCH(GRID, BLOCK, STREAM, LDS, KERNEL, BODY, ...) \
    ((void)(STREAM), aum::emu_launch(aum::grid_count(GRID), [&](int wg, auto* lds, auto* lds2) { (void)wg; (void)lds; (void)lds2; BODY; }, AUM_UNPAREN LDS))
#else
typedef hipStream_t aum_stream_t;
static int launch_status() { return hipGetLastError() == hipSuccess ? AUM_OK : AUM_E_LAUNCH; }
static inline dim3 launch_grid(int64_t g) { return dim3((unsigned)g); }
static inline dim3 launch_grid(Grid2 g) { return dim3(g.x, g.y); }
#define AUM_LAUNCH(GRID, BLOCK, STREAM, LDS, KERNEL, BODY, ...) \
    ({ hipLaunchKernelGGL(KERNEL, aum::launch_grid(GRID), dim3(BLOCK), aum::lds_dyn_bytes LDS, (STREAM), __VA_ARGS__); aum::launch_status(); })
#endif

// f(std::true_type{}) or f(std::false_type{}); nests
template <class F> static inline int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// f(std::integral_constant<int, v>{}) for v among V...; AUM_E_UNSUPPORTED for any other value
template <int... V, class F> static inline int with_int(int v, F&& f) {
    int rc = AUM_E_UNSUPPORTED;
    (void)((v == V ? (rc = f(std::integral_constant<int, V>{}), true) : false) || ...);
    return rc;
}
// the worker of `dtype` (AUM_F32 / AUM_BF16, else AUM_F16: callers have checked the range) on the arguments
template <class... P, class... A> static inline int by_dtype(int dtype, int (*f32)(P...), int (*bf16)(P...), int (*f16)(P...), A&&... args) {
    switch (dtype) {
        case AUM_F32: return f32(args...);
        case AUM_BF16: return bf16(args...);
        default: return f16(args...);
    }
}
#define AUM_BY_DTYPE_T(DTYPE, FN, ...) aum::by_dtype((DTYPE), FN<float>, FN<bf16_t>, FN<f16_t>, __VA_ARGS__)         // templates of this object
#define AUM_BY_DTYPE_X(DTYPE, FN, ...) aum::by_dtype((DTYPE), FN##_f32, FN##_bf16, FN##_f16, __VA_ARGS__)            // the per-dtype objects' workers

}  // namespace aum
