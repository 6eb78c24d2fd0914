// aum_hip.hip -- device translation unit of libaum_hip.so (gfx950).  The library is compiled as several
// objects from this one file (build.py parts()): -DAUM_API_PART=1/2 with -DAUM_DTYPE_ONLY=0/1/2 give the channel-major scan
// forward / backward kernels per activation dtype, 5/6 the token-major scan forward / backward kernels per dtype, 4 the skinny
// projection kernels per 16-bit dtype, and -DAUM_API_PART=3 the extern "C" surface with every other kernel (conv, norm, frontend,
// streaming).  No torch headers, no host framework: plain HIP + the C ABI of include/aum_hip.h.
#include "aum_api.inc"
