// stream_park_kernels.h -- PARK / RESUME: the cache rows of several streaming sessions into one record each of a byte blob, and back, in
// one launch (include/aum_hip.h: aum_stream_park).  A session is a row of every pool tensor (per layer the conv window and the scan
// state, the sample tail of a raw-audio stream); by hand that is one indexed copy per tensor, 2 * depth + 1 launches each way.
//
// Unit = (session, tensor, 4 KiB chunk of the tensor's row), chunk fastest: a workgroup of 256 lanes moves 256 x 16 bytes, lane i the 16
// bytes at chunk * 4096 + 16 i of the row -- consecutive lanes on consecutive addresses on both sides.  `per_session` (the host's sum of
// the tensors' chunk counts) splits the workgroup index into session and chunk-of-session; the tensor is found by walking the chunk
// counts, at most AUM_PARK_MAX_TENSORS uniform steps on kernel arguments.
// Bounds: a lane copies only if its 16 bytes start inside row_bytes (a multiple of 16, so they also end inside); the pool side is
// base + row * row_stride + offset, the blob side blob + session * blob_stride + blob_off + offset.  Nothing else is addressed: the
// bytes between the rows of a strided tensor and between or behind the ranges of a record are neither read nor written.  A negative row
// is skipped; that the rows exist is the host's check.
// The copy is of 32-bit words as they are (no float ever forms: NaN payloads travel), plain C++ 16-byte vector loads and stores.
#pragma once
#include <stdint.h>
#include "../../include/aum_hip.h"
#include "wave.h"

namespace aum {

constexpr int PARK_THREADS = 256;
constexpr int64_t PARK_CHUNK = PARK_THREADS * 16;      // bytes a workgroup moves

typedef uint32_t park_u4 __attribute__((ext_vector_type(4)));

AUM_HOSTDEV int64_t park_chunks(int64_t row_bytes) { return (row_bytes + PARK_CHUNK - 1) / PARK_CHUNK; }

// the operand rules of aum_stream_park (aum_hip.stream_park_args_ok mirrors them rule for rule) -> AUM_OK and the chunks of one session
static inline int park_check(const AumParkArgs* a, int64_t* per_session) {
    if (!a || !a->rows || !a->blob) return AUM_E_NULL;
    if (a->n_tensors < 1 || a->n_tensors > AUM_PARK_MAX_TENSORS || a->n_sessions < 1 || (a->flags & ~AUM_PARK_RESTORE)) return AUM_E_UNSUPPORTED;
    for (int t = 0; t < a->n_tensors; ++t)
        if (!a->base[t]) return AUM_E_NULL;
    const bool restore = (a->flags & AUM_PARK_RESTORE) != 0;
    if (((uintptr_t)a->rows & 3) || ((uintptr_t)a->blob & 15) || (a->blob_stride & 15) || a->blob_stride < 0) return AUM_E_UNSUPPORTED;
    int64_t end = 0, chunks = 0;
    for (int t = 0; t < a->n_tensors; ++t) {
        if (((uintptr_t)a->base[t] | (uintptr_t)a->row_stride[t] | (uintptr_t)a->row_bytes[t] | (uintptr_t)a->blob_off[t]) & 15) return AUM_E_UNSUPPORTED;
        if (a->row_bytes[t] < 16 || a->row_stride[t] < a->row_bytes[t] || a->blob_off[t] < end) return AUM_E_UNSUPPORTED;
        if (a->row_bytes[t] > ((int64_t)1 << 40)) return AUM_E_UNSUPPORTED;      // keeps the sums below in range
        end = a->blob_off[t] + a->row_bytes[t];
        chunks += park_chunks(a->row_bytes[t]);
    }
    if (!(restore && a->blob_stride == 0) && end > a->blob_stride) return AUM_E_UNSUPPORTED;
    if (chunks * a->n_sessions > 0x7fffffff) return AUM_E_UNSUPPORTED;
    *per_session = chunks;
    return AUM_OK;
}

// lane `tid` of workgroup `wg`
AUM_DEV void park_lane(const AumParkArgs& a, int64_t per_session, int64_t wg, int tid) {
    const int64_t s = wg / per_session;
    int64_t chunk = wg - s * per_session;
    int t = 0;
    for (; t < a.n_tensors - 1; ++t) {
        const int64_t c = park_chunks(a.row_bytes[t]);
        if (chunk < c) break;
        chunk -= c;
    }
    const int64_t off = chunk * PARK_CHUNK + (int64_t)tid * 16;
    const int64_t row = a.rows[s];
    if (off >= a.row_bytes[t] || row < 0) return;
    char* pool = static_cast<char*>(a.base[t]) + row * a.row_stride[t] + off;
    char* rec = static_cast<char*>(a.blob) + s * a.blob_stride + a.blob_off[t] + off;
    if (a.flags & AUM_PARK_RESTORE) *reinterpret_cast<park_u4*>(pool) = *reinterpret_cast<const park_u4*>(rec);
    else *reinterpret_cast<park_u4*>(rec) = *reinterpret_cast<const park_u4*>(pool);
}

#ifdef AUM_EMU
static inline void park_wg(const AumParkArgs& a, int64_t per_session, int wg) {
    for (int tid = 0; tid < PARK_THREADS; ++tid) park_lane(a, per_session, wg, tid);
}
#else
__global__ __launch_bounds__(PARK_THREADS) void k_stream_park(AumParkArgs a, int64_t per_session) {
    park_lane(a, per_session, (int64_t)blockIdx.x, (int)threadIdx.x);
}
#endif

}  // namespace aum
