// hifigan_msd_abi.hpp - host side of the HiFi-GAN scale discriminator's stack (C ABI in include/dsv.h, section "HiFi-GAN scale discriminator stack";
// kernels in hifigan_msd.hpp); included at the end of dsd.hip.  Every entry point validates on the host and refuses with DSD_ERR_INVALID before any
// launch; nothing allocates, copies, synchronises or reads a device value: argument checks, launches on the caller's stream with by-value
// arguments, hipGetLastError.
#include "hifigan_msd.hpp"
#include "voc_train_host.hpp"

// the five grouped layers of DiscriminatorS (hifigan.py:265-269) and how the kernels tile them
struct HgsGeom {
    int Ci, Co, S, G;
    int mt_f, e_f;          // forward: MFMA rows per block, k steps per A load (rows co_g, channels ci_g)
    int mt_b, e_b;          // data gradient (rows ci_g, channels co_g)
};
static const HgsGeom kHgsGeoms[5] = {
    {128, 128, 2, 4, 32, 4, 32, 4},        // 32 x 32 per group
    {128, 256, 2, 16, 16, 2, 16, 4},       // 16 x 8: the data gradient's 8 rows sit in a 16-row block
    {256, 512, 4, 16, 32, 4, 16, 4},       // 32 x 16
    {512, 1024, 4, 16, 32, 4, 32, 4},      // 64 x 32
    {1024, 1024, 1, 16, 32, 4, 32, 4},     // 64 x 64
};
static const HgsGeom* hgs_geom(int Ci, int Co, int S, int G) {
    for (const HgsGeom& g : kHgsGeoms)
        if (g.Ci == Ci && g.Co == Co && g.S == S && g.G == G) return &g;
    return nullptr;
}
static int hgs_check_geom(const char* who, int Ci, int Co, int S, int G, const HgsGeom** out) {
    *out = hgs_geom(Ci, Co, S, G);
    if (!*out)
        return fail(DSD_ERR_INVALID,
                    "%s: (Ci=%d, Co=%d, stride=%d, groups=%d) is none of the grouped layers (128, 128, 2, 4), (128, 256, 2, 16), (256, 512, 4, 16), "
                    "(512, 1024, 4, 16), (1024, 1024, 1, 16)", who, Ci, Co, S, G);
    return DSD_OK;
}
static int hgs_out_len(int L, int S) { return (L - 1) / S + 1; }    // K = 41, padding 20
static int hgs_log2(int s) { return s == 4 ? 2 : s == 2 ? 1 : 0; }
// an operand that is only read (`in`, may be null: skipped) against a range the call writes; inputs may overlap one another
static int hgs_disjoint(const char* who, const float* in, int64_t n_in, const float* out, int64_t n_out) {
    if (!in || !out) return DSD_OK;
    return voc_check_disjoint(who, in, n_in, out, n_out);
}
// B <= 65535 is grid z; B * C * L stays below 2^40 floats
static int hgs_check_shape(const char* who, int B, int L) { return voc_check_shape(who, B, L); }

extern "C" int32_t dsv_hgs_out_len(int32_t L, int32_t stride) { return (L < 1 || (stride != 1 && stride != 2 && stride != 4)) ? -1 : hgs_out_len(L, stride); }

// ---- first layer ------------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t dsv_hgs_first_workspace_floats(int32_t B, int32_t T, int32_t C) {
    if (!voc_shape_ok(B, T) || C < 1 || C > 65535) return -1;
    return (((int64_t)B * T + kHgpEdgeSplit - 1) / kHgpEdgeSplit) * C * (kHgsFirstK + 1);
}

extern "C" int dsv_hgs_first(const float* x, const float* w, const float* bias, float* out, int32_t B, int32_t C, int32_t T, int64_t ld_x, float slope,
                             void* stream) {
    if (!x || !w || !out) return fail(DSD_ERR_INVALID, "dsv_hgs_first: null argument");
    DSD_TRY(hgs_check_shape("dsv_hgs_first", B, T));
    DSD_TRY(voc_check_slope("dsv_hgs_first", slope));
    DSD_TRY(voc_check_grid_channels("dsv_hgs_first", C));
    DSD_TRY(voc_check_row_stride("dsv_hgs_first", ld_x, T));
    DSD_TRY(voc_check_disjoint("dsv_hgs_first", x, (B - 1) * ld_x + T, out, (int64_t)B * C * T));
    DSD_TRY(hgs_disjoint("dsv_hgs_first", w, (int64_t)C * kHgsFirstK, out, (int64_t)B * C * T));
    DSD_TRY(hgs_disjoint("dsv_hgs_first", bias, C, out, (int64_t)B * C * T));
    hipLaunchKernelGGL(k_hgs_first, dim3((unsigned)((T + 255) / 256), (unsigned)C, (unsigned)B), dim3(256), 0, (hipStream_t)stream, x, w, bias, out, C, T,
                       (long long)ld_x, slope);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgs_first_backward(const float* g0, const float* x, const float* w, float* workspace, float* dw, float* db, float* dx, int32_t B,
                                      int32_t C, int32_t T, int64_t ld_x, void* stream) {
    if (!g0 || !x || !w || !workspace || !dw) return fail(DSD_ERR_INVALID, "dsv_hgs_first_backward: null argument");
    DSD_TRY(hgs_check_shape("dsv_hgs_first_backward", B, T));
    DSD_TRY(voc_check_grid_channels("dsv_hgs_first_backward", C));
    DSD_TRY(voc_check_row_stride("dsv_hgs_first_backward", ld_x, T));
    const int64_t npos = (int64_t)B * T;
    const int64_t nsplit = (npos + kHgpEdgeSplit - 1) / kHgpEdgeSplit;
    if (nsplit > 65535) return fail(DSD_ERR_INVALID, "dsv_hgs_first_backward: %lld splits exceed 65535 workgroups", (long long)nsplit);
    {   // every range the call reads against every range it writes, and the written ranges against one another
        const int64_t n_ws = nsplit * C * (kHgsFirstK + 1), n_g = (int64_t)B * C * T, n_x = (B - 1) * ld_x + T, n_w = (int64_t)C * kHgsFirstK;
        const float* outs[4] = {workspace, dw, db, dx};
        const int64_t n_out[4] = {n_ws, n_w, C, (int64_t)B * T};
        for (int i = 0; i < 4; ++i) {
            DSD_TRY(hgs_disjoint("dsv_hgs_first_backward", g0, n_g, outs[i], n_out[i]));
            DSD_TRY(hgs_disjoint("dsv_hgs_first_backward", x, n_x, outs[i], n_out[i]));
            DSD_TRY(hgs_disjoint("dsv_hgs_first_backward", w, n_w, outs[i], n_out[i]));
            for (int k = i + 1; k < 4; ++k) DSD_TRY(hgs_disjoint("dsv_hgs_first_backward", outs[i], n_out[i], outs[k], n_out[k]));
        }
    }
    hipLaunchKernelGGL(k_hgs_first_wgrad, dim3((unsigned)C, (unsigned)nsplit), dim3(256), 0, (hipStream_t)stream, g0, x, workspace, C, T, (long long)ld_x,
                       (long long)npos);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_hgp_edge_reduce, dim3((unsigned)((C * (kHgsFirstK + 1) + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                       dw, db, (int)nsplit, C, kHgsFirstK, 1);
    HIP_TRY(hipGetLastError());
    if (dx) {
        hipLaunchKernelGGL(k_hgs_first_dx, dim3((unsigned)((T + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, g0, w, dx, C, T);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}

// ---- packing ----------------------------------------------------------------------------------------------------------------------------------------
// data gradient, input phase r: first tap k0 = (r + 20) mod s, number of taps, and d = (r + 20 - k0) / s
static void hgs_phase(int S, int r, int* k0, int* nt, int* d) {
    *k0 = (r + kHgsPad) % S;
    *nt = (kHgsK - 1 - *k0) / S + 1;
    *d = (r + kHgsPad - *k0) / S;
}
static void hgs_pack_params(const HgsGeom& ge, int bwd, HgsPackParams* p) {
    const int co_g = ge.Co / ge.G, ci_g = ge.Ci / ge.G;
    p->G = ge.G; p->co_g = co_g; p->ci_g = ci_g; p->S = ge.S; p->bwd = bwd;
    p->MT = bwd ? ge.mt_b : ge.mt_f; p->E = bwd ? ge.e_b : ge.e_f;
    const int rows = bwd ? ci_g : co_g, kc = bwd ? co_g : ci_g;
    p->RB = (rows + p->MT - 1) / p->MT;
    p->nphase = bwd ? ge.S : 1;
    p->off[0] = 0;
    for (int r = 0; r < p->nphase; ++r) {
        int d;
        if (bwd) hgs_phase(ge.S, r, &p->k0[r], &p->nt[r], &d);
        else { p->k0[r] = 0; p->nt[r] = kHgsK; }
        p->off[r + 1] = p->off[r] + (long long)ge.G * p->RB * p->MT * kc * p->nt[r];
    }
}

extern "C" int64_t dsv_hgs_packed_floats(int32_t Ci, int32_t Co, int32_t stride, int32_t groups, int32_t dgrad) {
    const HgsGeom* ge = hgs_geom(Ci, Co, stride, groups);
    if (!ge || (dgrad != 0 && dgrad != 1)) return -1;
    HgsPackParams p{};
    hgs_pack_params(*ge, dgrad, &p);
    return p.off[p.nphase];
}

extern "C" int dsv_hgs_pack(const float* w, float* packed, int32_t Ci, int32_t Co, int32_t stride, int32_t groups, int32_t dgrad, void* stream) {
    if (!w || !packed) return fail(DSD_ERR_INVALID, "dsv_hgs_pack: null argument");
    const HgsGeom* ge;
    DSD_TRY(hgs_check_geom("dsv_hgs_pack", Ci, Co, stride, groups, &ge));
    if (dgrad != 0 && dgrad != 1) return fail(DSD_ERR_INVALID, "dsv_hgs_pack: dgrad=%d must be 0 or 1", dgrad);
    if ((uintptr_t)packed & 15) return fail(DSD_ERR_INVALID, "dsv_hgs_pack: the packed buffer must be aligned to 16 bytes");
    HgsPackParams p{};
    hgs_pack_params(*ge, dgrad, &p);
    DSD_TRY(voc_check_disjoint("dsv_hgs_pack", w, (int64_t)Co * (Ci / groups) * kHgsK, packed, p.off[p.nphase]));
    p.w = w; p.out = packed;
    hipLaunchKernelGGL(k_hgs_pack, dim3((unsigned)((p.off[p.nphase] + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

// ---- forward and data gradient ----------------------------------------------------------------------------------------------------------------------
static int hgs_launch_gemm(HgsGemmParams& p, int MT, int E, int max_taps, int max_cols, int nphase, int B, hipStream_t s) {
    const int NQ = (4 / p.RB) * MT, ss = 1 << p.sh;
    p.PL = NQ + (max_taps - 1) / ss + 1;
    p.CS = ss * p.PL;
    if (MT == 16) p.CS += ((16 - p.CS % 32) + 32) % 32;         // the four k groups of a 16 x 16 x 4 step on different banks
    else p.CS += ((1 - p.CS % 2) + 2) % 2;
    const size_t lds = (size_t)p.kc_g * p.CS * sizeof(float);
    const dim3 grid((unsigned)((max_cols + NQ - 1) / NQ), (unsigned)(p.G * nphase), (unsigned)B);
    if (MT == 32 && E == 4) hipLaunchKernelGGL((k_hgs_gemm<32, 4>), grid, dim3(kThreads), lds, s, p);
    else if (MT == 16 && E == 2) hipLaunchKernelGGL((k_hgs_gemm<16, 2>), grid, dim3(kThreads), lds, s, p);
    else if (MT == 16 && E == 4) hipLaunchKernelGGL((k_hgs_gemm<16, 4>), grid, dim3(kThreads), lds, s, p);
    else return fail(DSD_ERR_INVALID, "dsv_hgs_gconv: no kernel for %d-row blocks with %d k steps per load", MT, E);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

extern "C" int dsv_hgs_gconv(const float* x, const float* w_packed, const float* bias, float* out, int32_t B, int32_t Ci, int32_t Co, int32_t L,
                             int32_t stride, int32_t groups, float slope, void* stream) {
    if (!x || !w_packed || !out) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv: null argument");
    const HgsGeom* ge;
    DSD_TRY(hgs_check_geom("dsv_hgs_gconv", Ci, Co, stride, groups, &ge));
    DSD_TRY(hgs_check_shape("dsv_hgs_gconv", B, L));
    DSD_TRY(voc_check_slope("dsv_hgs_gconv", slope));
    if ((uintptr_t)w_packed & 15) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv: the packed weights must be aligned to 16 bytes");
    const int Lo = hgs_out_len(L, stride), co_g = Co / groups, ci_g = Ci / groups;
    DSD_TRY(voc_check_disjoint("dsv_hgs_gconv", x, (int64_t)B * Ci * L, out, (int64_t)B * Co * Lo));
    DSD_TRY(hgs_disjoint("dsv_hgs_gconv", w_packed, dsv_hgs_packed_floats(Ci, Co, stride, groups, 0), out, (int64_t)B * Co * Lo));
    DSD_TRY(hgs_disjoint("dsv_hgs_gconv", bias, Co, out, (int64_t)B * Co * Lo));
    HgsGemmParams p{};
    p.src = x; p.bias = bias; p.dst = out;
    p.G = groups; p.Csrc = Ci; p.Lsrc = L; p.kc_g = ci_g; p.Cdst = Co; p.Ldst = Lo; p.rows_g = co_g; p.RB = co_g / ge->mt_f;
    p.sh = hgs_log2(stride); p.So = 1; p.slope = slope; p.bwd = 0;
    p.ph[0].wp = w_packed; p.ph[0].ntaps = kHgsK; p.ph[0].org = -kHgsPad; p.ph[0].ro = 0; p.ph[0].ncols = Lo;
    return hgs_launch_gemm(p, ge->mt_f, ge->e_f, kHgsK, Lo, 1, B, (hipStream_t)stream);
}

extern "C" int dsv_hgs_gconv_dgrad(const float* g, const float* w_packed, const float* cot, const float* saved, float* out, int32_t B, int32_t Ci,
                                   int32_t Co, int32_t L, int32_t stride, int32_t groups, float slope, void* stream) {
    if (!g || !w_packed || !out) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_dgrad: null argument");
    const HgsGeom* ge;
    DSD_TRY(hgs_check_geom("dsv_hgs_gconv_dgrad", Ci, Co, stride, groups, &ge));
    DSD_TRY(hgs_check_shape("dsv_hgs_gconv_dgrad", B, L));
    DSD_TRY(voc_check_slope("dsv_hgs_gconv_dgrad", slope));
    if ((uintptr_t)w_packed & 15) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_dgrad: the packed weights must be aligned to 16 bytes");
    const int Lo = hgs_out_len(L, stride), co_g = Co / groups, ci_g = Ci / groups;
    DSD_TRY(voc_check_disjoint("dsv_hgs_gconv_dgrad", g, (int64_t)B * Co * Lo, out, (int64_t)B * Ci * L));
    DSD_TRY(hgs_disjoint("dsv_hgs_gconv_dgrad", w_packed, dsv_hgs_packed_floats(Ci, Co, stride, groups, 1), out, (int64_t)B * Ci * L));
    DSD_TRY(hgs_disjoint("dsv_hgs_gconv_dgrad", cot, (int64_t)B * Ci * L, out, (int64_t)B * Ci * L));
    DSD_TRY(hgs_disjoint("dsv_hgs_gconv_dgrad", saved, (int64_t)B * Ci * L, out, (int64_t)B * Ci * L));
    HgsPackParams pk{};
    hgs_pack_params(*ge, 1, &pk);
    HgsGemmParams p{};
    p.src = g; p.cot = cot; p.saved = saved; p.dst = out;
    p.G = groups; p.Csrc = Co; p.Lsrc = Lo; p.kc_g = co_g; p.Cdst = Ci; p.Ldst = L; p.rows_g = ci_g; p.RB = pk.RB;
    p.sh = 0; p.So = stride; p.slope = slope; p.bwd = 1;
    int max_cols = 0, max_taps = 0;
    for (int r = 0; r < stride; ++r) {
        int k0, nt, d;
        hgs_phase(stride, r, &k0, &nt, &d);
        HgsPhase& ph = p.ph[r];
        ph.wp = w_packed + pk.off[r]; ph.ntaps = nt; ph.org = d - (nt - 1); ph.ro = r;
        ph.ncols = L > r ? (L - r + stride - 1) / stride : 0;       // input positions s m + r < L
        max_cols = std::max(max_cols, ph.ncols);
        max_taps = std::max(max_taps, nt);
    }
    return hgs_launch_gemm(p, ge->mt_b, ge->e_b, max_taps, max_cols, stride, B, (hipStream_t)stream);
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------
// Units of 32 positions of one batch row; a split is `upc` consecutive units, 16 (kSplitK positions) at least and doubled until the launch has at
// most 1024 workgroups: the output tiles alone (groups x ci_g / 8: 16 to 128) never fill the chip's 256 compute units
static void hgs_wgrad_plan(const HgsGeom& ge, int B, int Lo, int* nst, int* upc, int* nsplit) {
    const int tiles = ge.G * (ge.Ci / ge.G / kHgsWgCi);
    *nst = (Lo + kHgsWgPos - 1) / kHgsWgPos;
    const int64_t units = (int64_t)B * *nst;
    int64_t u = kSplitK / kHgsWgPos;
    while ((units + u - 1) / u * tiles > 1024) u *= 2;
    *upc = (int)std::min<int64_t>(u, units);
    *nsplit = (int)((units + *upc - 1) / *upc);
}
extern "C" int32_t dsv_hgs_wgrad_splits(int32_t B, int32_t Ci, int32_t Co, int32_t L_out, int32_t stride, int32_t groups) {
    const HgsGeom* ge = hgs_geom(Ci, Co, stride, groups);
    if (!ge || !voc_shape_ok(B, L_out)) return -1;
    int nst, upc, nsplit;
    hgs_wgrad_plan(*ge, B, L_out, &nst, &upc, &nsplit);
    return nsplit;
}
extern "C" int64_t dsv_hgs_wgrad_workspace_floats(int32_t B, int32_t Ci, int32_t Co, int32_t L_out, int32_t stride, int32_t groups) {
    const int n = dsv_hgs_wgrad_splits(B, Ci, Co, L_out, stride, groups);
    if (n < 0) return -1;
    return n == 1 ? 0 : (int64_t)n * Co * (Ci / groups) * kHgsK;
}

extern "C" int dsv_hgs_gconv_wgrad(const float* g, const float* x, float* workspace, float* dw, float* db, int32_t B, int32_t Ci, int32_t Co, int32_t L,
                                   int32_t stride, int32_t groups, void* stream) {
    if (!g || !x || !dw) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_wgrad: null argument");
    const HgsGeom* ge;
    DSD_TRY(hgs_check_geom("dsv_hgs_gconv_wgrad", Ci, Co, stride, groups, &ge));
    DSD_TRY(hgs_check_shape("dsv_hgs_gconv_wgrad", B, L));
    const int Lo = hgs_out_len(L, stride), co_g = Co / groups, ci_g = Ci / groups;
    int nst, upc, nsplit;
    hgs_wgrad_plan(*ge, B, Lo, &nst, &upc, &nsplit);
    if ((int64_t)B * nst > (1 << 30)) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_wgrad: B * ceil(L_out / 32) = %lld exceeds 2^30", (long long)B * nst);
    if (nsplit > 1 && !workspace) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_wgrad: %d splits need the workspace", nsplit);
    if (nsplit > 65535) return fail(DSD_ERR_INVALID, "dsv_hgs_gconv_wgrad: %d splits exceed 65535 workgroups", nsplit);
    const int64_t n = (int64_t)Co * ci_g * kHgsK;
    DSD_TRY(voc_check_disjoint("dsv_hgs_gconv_wgrad", g, (int64_t)B * Co * Lo, dw, n));
    DSD_TRY(voc_check_disjoint("dsv_hgs_gconv_wgrad", x, (int64_t)B * Ci * L, dw, n));
    {
        const float* outs[3] = {nsplit > 1 ? workspace : nullptr, dw, db};
        const int64_t n_out[3] = {(int64_t)nsplit * n, n, Co};
        for (int i = 0; i < 3; ++i) {
            DSD_TRY(hgs_disjoint("dsv_hgs_gconv_wgrad", g, (int64_t)B * Co * Lo, outs[i], n_out[i]));
            DSD_TRY(hgs_disjoint("dsv_hgs_gconv_wgrad", x, (int64_t)B * Ci * L, outs[i], n_out[i]));
            for (int k = i + 1; k < 3; ++k) DSD_TRY(hgs_disjoint("dsv_hgs_gconv_wgrad", outs[i], n_out[i], outs[k], n_out[k]));
        }
    }
    HgsWgradParams p{};
    p.g = g; p.x = x; p.out = nsplit > 1 ? workspace : dw;
    p.B = B; p.Co = Co; p.Ci = Ci; p.co_g = co_g; p.ci_g = ci_g; p.Lout = Lo; p.Lin = L; p.S = stride;
    p.nst = nst; p.units = B * nst; p.upc = upc;
    const int WL = (kHgsWgPos - 1) * stride + kHgsK;
    p.CSW = WL + ((9 - WL % 32) + 32) % 32;
    const dim3 grid((unsigned)(ci_g / kHgsWgCi), (unsigned)groups, (unsigned)nsplit);
    if (co_g == 16) hipLaunchKernelGGL((k_hgs_wgrad<16, 1>), grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    else if (co_g == 32) hipLaunchKernelGGL((k_hgs_wgrad<32, 1>), grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((k_hgs_wgrad<32, 2>), grid, dim3(kThreads), 0, (hipStream_t)stream, p);
    HIP_TRY(hipGetLastError());
    if (nsplit > 1) {
        hipLaunchKernelGGL(k_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, dw, (int)n, nsplit);
        HIP_TRY(hipGetLastError());
    }
    if (db) {
        hipLaunchKernelGGL(k_hgp_bias_grad, dim3((unsigned)Co), dim3(256), 0, (hipStream_t)stream, g, db, B, Co, Lo);
        HIP_TRY(hipGetLastError());
    }
    return DSD_OK;
}
