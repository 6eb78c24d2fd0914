// xdt_fwd_body.inc -- the body of the x_proj / dt_proj forward pass (xdt_kernels.h), as TEXT: included inside k_xdt_tm_fwd and inside
// k_stream_block (stream_block_kernels.h), so both kernels run one and the same statement sequence and the first stays, instruction for
// instruction, the kernel it was (as an inlined function the same statements came out two registers heavier at 8 waves).
// The including scope provides: template constants BF16, KS, NW, NC, SOFTPLUS;  AumXdtArgs g;  char* lds (lds_bytes(XDT_MAX_DIM, NW) bytes of
// LDS, 16-byte aligned);  XDT_BODY_WG, the workgroup's index in the token stream (NW * XDT_TOK_W tokens each).
    constexpr int NCF = (NC + 15) / 16;
    constexpr int XP = NC == 80 ? 176 : 144;             // bytes per tile row: an odd number of 16-byte chunks (conflict-free fragment reads); 56, 48: 9
    static_assert(NC % 8 == 0 && NCF * 32 <= XP && XP <= aumx::XP, "tile row holds every fragment column");
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int rho = lane & 15, kg = lane >> 4;
    const int E = g.dim, KH = E / 2, SP = slab_pitch(KH);
    char* slab = lds;
    char* xt = lds + slab_bytes(E) + w * XT_BYTES;
    const int64_t t0 = (int64_t)XDT_BODY_WG * (NW * XDT_TOK_W) + w * XDT_TOK_W;
    const s8v zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const char* ub = static_cast<const char*>(g.u);
    bool tok_ok[NTF];
    const char* urow[NTF];
    for (int tf = 0; tf < NTF; ++tf) {
        tok_ok[tf] = t0 + tf * 16 + rho < g.ntok;
        urow[tf] = ub + ((t0 + tf * 16 + rho) * g.ldu + kg * 16) * 2;
    }

    f4v acc[NTF][NCF];
#pragma unroll
    for (int tf = 0; tf < NTF; ++tf)
#pragma unroll
        for (int f = 0; f < NCF; ++f) acc[tf][f] = f4v{0.f, 0.f, 0.f, 0.f};

    // ---- stage A: x_dbl = u . W_x^T, K in two halves of W_x through LDS -------------------------------------------------------
    auto load_u = [&](int k0, s8v (&uf)[NTF][2]) {
#pragma unroll
        for (int tf = 0; tf < NTF; ++tf) {
            uf[tf][0] = tok_ok[tf] ? *reinterpret_cast<const s8v*>(urow[tf] + (int64_t)k0 * 2) : zero;
            uf[tf][1] = tok_ok[tf] ? *reinterpret_cast<const s8v*>(urow[tf] + (int64_t)k0 * 2 + 16) : zero;
        }
    };
    // conv_out rows arrive through a ring of four register sets indexed by the (unrolled) step: a set is refilled, four steps ahead, right
    // after the MFMAs that read it were issued.  (Rotating three sets through register copies -- the first version -- made every copy wait
    // for its load: the prefetch distance collapsed to one step.)
    const int nsteps = KH / 64, total = E / 64;               // steps per K-half; dim % 128 == 0 (xdt_fwd_shape_ok) -> total is even
    s8v ur[4][NTF][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < total) load_u(j * 64, ur[j]);
    const char* wrd = slab + rho * SP + kg * 32;              // + f * 16 rows, + step-in-half * 128 bytes
    for (int s0 = 0; s0 < total; s0 += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = s0 + j;
            if (j == 2 && s >= total) break;                  // dim % 256 == 128: the last round has two steps (sets 2, 3 were not refilled)
            if (s == 0 || s == nsteps) {                      // a K-half of W_x through LDS
                __syncthreads();                              // everybody is done with the previous contents of the slab
                stage_rows<NW * 64>(slab, SP, static_cast<const char*>(g.wx) + (int64_t)(s / nsteps) * KH * 2, (int64_t)g.ldwx * 2, NC, KH / 8, tid);
                __syncthreads();
            }
            const int sl = s >= nsteps ? s - nsteps : s;
#pragma unroll
            for (int f = 0; f < NCF; ++f) {
                const s8v w0 = *reinterpret_cast<const s8v*>(wrd + f * 16 * SP + sl * 128);
                const s8v w1 = *reinterpret_cast<const s8v*>(wrd + f * 16 * SP + sl * 128 + 16);
#pragma unroll
                for (int tf = 0; tf < NTF; ++tf) {
                    acc[tf][f] = mfma<BF16>(w0, ur[j][tf][0], acc[tf][f]);
                    acc[tf][f] = mfma<BF16>(w1, ur[j][tf][1], acc[tf][f]);
                }
            }
            if (s + 4 < total) load_u((s + 4) * 64, ur[j]);
        }
    }
    // ---- the wave's x_dbl tile: rounded once, [token][column] in LDS; x_dbl leaves from there in 16-byte pieces --------------------
    // lane (kg, token rho) holds columns 16 f + 4 kg + r of token fragment tf
#pragma unroll
    for (int tf = 0; tf < NTF; ++tf)
#pragma unroll
        for (int f = 0; f < NCF; ++f) {
            u2v v;
            v.x = pack2<BF16>(acc[tf][f][0], acc[tf][f][1]);
            v.y = pack2<BF16>(acc[tf][f][2], acc[tf][f][3]);
            *reinterpret_cast<u2v*>(xt + (tf * 16 + rho) * XP + (f * 16 + kg * 4) * 2) = v;
        }
    __builtin_amdgcn_s_waitcnt(0xc07f);                              // lgkmcnt(0): the wave's own LDS writes have landed (nobody else reads this tile)
    {
        char* xo = static_cast<char*>(g.x_dbl);
        constexpr int PIECES = NC * 2 / 16;                          // 10 / 7 / 6 per token row
        for (int idx = lane; idx < XDT_TOK_W * PIECES; idx += 64) {
            const int tk = idx / PIECES, pc = idx - tk * PIECES;
            if (t0 + tk < g.ntok)
                *reinterpret_cast<u4v*>(xo + ((t0 + tk) * g.ldx) * 2 + pc * 16) = *reinterpret_cast<const u4v*>(xt + tk * XP + pc * 16);
        }
    }
    // ---- stage B: delta = x_dbl[:, :R] . W_dt^T, the channels in two halves of W_dt through the same LDS space -------------------
    s8v xf[NTF][KS];
#pragma unroll
    for (int tf = 0; tf < NTF; ++tf)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k = ks * 32 + kg * 8;
            xf[tf][ks] = k < g.rank ? *reinterpret_cast<const s8v*>(xt + (tf * 16 + rho) * XP + k * 2) : zero;
        }
    const bool k_ok[2] = {kg * 8 < g.rank, 32 + kg * 8 < g.rank};
    const int CH = E / 2, wchunks = g.rank / 8;
    char* ob = static_cast<char*>(g.delta) + ((t0 + rho) * g.ldd + kg * 8) * 2;
    const int64_t otf = (int64_t)16 * g.ldd * 2;
    // fragment j of a channel pair reads weight rows c0 + 8 (rho >> 2) + 4 j + (rho & 3): accumulator rows 4 kg + r of fragments 0, 1 are
    // channels c0 + 8 kg + 0..7
    const char* wdr = slab + ((rho >> 2) * 8 + (rho & 3)) * WDP + kg * 16;
    // SOFTPLUS: the half's CH bias values behind its W_dt rows (CH * WDP + 4 CH <= slab_bytes(E)), one 16-byte piece per thread; this lane's
    // eight channels of pair p at floats p * 32 + 8 kg
    static_assert((XDT_MAX_DIM / 2) / 4 <= XDT_WAVES_MIN * 64 && (XDT_MAX_DIM / 2) * (WDP + 4) <= slab_bytes(XDT_MAX_DIM), "bias staging");
    const float* bl = reinterpret_cast<const float*>(slab + CH * WDP) + kg * 8;
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        f4v bv = {0.f, 0.f, 0.f, 0.f};
        if (SOFTPLUS && tid < CH / 4 && g.delta_bias) bv = *reinterpret_cast<const f4v*>(g.delta_bias + half * CH + tid * 4);
        stage_rows<NW * 64>(slab, WDP, static_cast<const char*>(g.wdt) + (int64_t)half * CH * g.ldwdt * 2, (int64_t)g.ldwdt * 2, CH, wchunks, tid);
        if (SOFTPLUS && tid < CH / 4) *reinterpret_cast<f4v*>(slab + CH * WDP + tid * 16) = bv;
        __syncthreads();
        const int npairs = CH / 32;
#pragma unroll 2
        for (int p = 0; p < npairs; ++p) {
            s8v wf[2][KS];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    wf[j][ks] = k_ok[ks] ? *reinterpret_cast<const s8v*>(wdr + (p * 32 + j * 4) * WDP + ks * 64) : zero;
#pragma unroll
            for (int tf = 0; tf < NTF; ++tf) {
                f4v a2[2] = {f4v{0.f, 0.f, 0.f, 0.f}, f4v{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) a2[j] = mfma<BF16>(wf[j][ks], xf[tf][ks], a2[j]);
                if (tok_ok[tf]) {
                    u4v o;
                    if constexpr (SOFTPLUS) {       // the scans' softplus (SSI:106-107) on pairs: x > 20 passes, d == 0 keeps exp(x)
                        const f4v b0 = *reinterpret_cast<const f4v*>(bl + p * 32), b1 = *reinterpret_cast<const f4v*>(bl + p * 32 + 4);
                        const aum::vf2 d0 = aum::vsoftplus2(aum::vf2{a2[0][0], a2[0][1]} + aum::vf2{b0[0], b0[1]});
                        const aum::vf2 d1 = aum::vsoftplus2(aum::vf2{a2[0][2], a2[0][3]} + aum::vf2{b0[2], b0[3]});
                        const aum::vf2 d2 = aum::vsoftplus2(aum::vf2{a2[1][0], a2[1][1]} + aum::vf2{b1[0], b1[1]});
                        const aum::vf2 d3 = aum::vsoftplus2(aum::vf2{a2[1][2], a2[1][3]} + aum::vf2{b1[2], b1[3]});
                        o.x = pack2<BF16>(d0[0], d0[1]);
                        o.y = pack2<BF16>(d1[0], d1[1]);
                        o.z = pack2<BF16>(d2[0], d2[1]);
                        o.w = pack2<BF16>(d3[0], d3[1]);
                    } else {
                        o.x = pack2<BF16>(a2[0][0], a2[0][1]);
                        o.y = pack2<BF16>(a2[0][2], a2[0][3]);
                        o.z = pack2<BF16>(a2[1][0], a2[1][1]);
                        o.w = pack2<BF16>(a2[1][2], a2[1][3]);
                    }
                    *reinterpret_cast<u4v*>(ob + tf * otf + ((int64_t)half * CH + p * 32) * 2) = o;
                }
            }
        }
    }
