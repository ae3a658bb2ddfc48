// voc_optim_abi.hpp - the entry points of include/dsv.h, section "Vocoder optimisers" (kernels: voc_optim.hpp); included behind dsd.hip's fail().
// The entry points take HOST arrays of device pointers and element counts and split them over as many launches as the tables need.
#pragma once
#include "voc_optim.hpp"

// the table capacity in use: the kernels' own, or less (dsv_mt_set_table_limit - a list then crosses launch seams at a size a test can afford)
static int g_mt_tensors = kMtMaxTensors, g_mt_chunks = kMtMaxChunks;

static int64_t mt_chunks_of(int64_t n) { return (n + kMtChunk - 1) / kMtChunk; }

static int mt_check_counts(const char* who, const int64_t* n, int64_t count) {
    if (!n || count < 1 || count > ((int64_t)1 << 24)) return fail(DSD_ERR_INVALID, "%s: bad argument (count=%lld must be in [1, 2^24] with its arrays)", who, (long long)count);
    for (int64_t i = 0; i < count; ++i)
        if (n[i] < 1 || n[i] > ((int64_t)1 << 40)) return fail(DSD_ERR_INVALID, "%s: bad shape (n[%lld]=%lld must be in [1, 2^40])", who, (long long)i, (long long)n[i]);
    return DSD_OK;
}

static int mt_check_pointers(const char* who, const char* name, const void* const* a, int64_t count) {
    if (!a) return fail(DSD_ERR_INVALID, "%s: null argument (%s)", who, name);
    for (int64_t i = 0; i < count; ++i) {
        if (!a[i]) return fail(DSD_ERR_INVALID, "%s: null pointer (%s[%lld])", who, name, (long long)i);
        if ((uintptr_t)a[i] & 3) return fail(DSD_ERR_INVALID, "%s: %s[%lld] is not aligned to a float", who, name, (long long)i);
    }
    return DSD_OK;
}

// Walks the list and hands out launches: fill(slot, i) enters tensor i under `slot`, launch(chunks, n_chunks, first_global_chunk) runs one table.
template <class Fill, class Launch>
static int mt_split(const int64_t* n, int64_t count, Fill fill, Launch launch) {
    MtChunks c{};
    int nt = 0, nc = 0;
    int64_t first = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t total = mt_chunks_of(n[i]);
        int64_t done = 0;
        while (done < total) {
            if (nt == g_mt_tensors || nc == g_mt_chunks) {
                DSD_TRY(launch(c, nc, first));
                first += nc;
                nt = nc = 0;
            }
            const int slot = nt++;
            fill(slot, i);
            const int64_t take = std::min<int64_t>(total - done, g_mt_chunks - nc);
            for (int64_t k = 0; k < take; ++k, ++nc) {
                c.chunk[nc] = (int)(done + k);
                c.tensor[nc] = (unsigned char)slot;
            }
            done += take;
        }
    }
    if (nc) DSD_TRY(launch(c, nc, first));
    return DSD_OK;
}

extern "C" int32_t dsv_mt_chunk_floats(void) { return kMtChunk; }
extern "C" int32_t dsv_mt_table_tensors(void) { return g_mt_tensors; }
extern "C" int32_t dsv_mt_table_chunks(void) { return g_mt_chunks; }

extern "C" int dsv_mt_set_table_limit(int32_t tensors, int32_t chunks) {
    if (tensors < 0 || tensors > kMtMaxTensors || chunks < 0 || chunks > kMtMaxChunks)
        return fail(DSD_ERR_INVALID, "dsv_mt_set_table_limit: tensors in [0, %d], chunks in [0, %d] (0: the kernels' capacity)", kMtMaxTensors, kMtMaxChunks);
    g_mt_tensors = tensors ? tensors : kMtMaxTensors;
    g_mt_chunks = chunks ? chunks : kMtMaxChunks;
    return DSD_OK;
}

extern "C" int64_t dsv_mt_workspace_floats(const int64_t* n, int64_t count) {
    if (!n || count < 1 || count > ((int64_t)1 << 24)) return -1;
    int64_t chunks = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (n[i] < 1 || n[i] > ((int64_t)1 << 40)) return -1;
        chunks += mt_chunks_of(n[i]);
    }
    return 2 * chunks;                                       // one float64 partial per chunk
}

extern "C" int dsv_mt_grad_norm(const float* const* g, const int64_t* n, int64_t count, double max_norm, float* workspace, int64_t workspace_floats,
                                float* out2, void* stream) {
    DSD_TRY(mt_check_counts("dsv_mt_grad_norm", n, count));
    DSD_TRY(mt_check_pointers("dsv_mt_grad_norm", "g", (const void* const*)g, count));
    if (!workspace || !out2) return fail(DSD_ERR_INVALID, "dsv_mt_grad_norm: null argument");
    if ((uintptr_t)out2 & 3) return fail(DSD_ERR_INVALID, "dsv_mt_grad_norm: out2 is not aligned to a float");
    DSD_TRY(voc_check_f64_workspace("dsv_mt_grad_norm", workspace, "it holds float64 partial sums"));
    if (!(max_norm >= 0)) return fail(DSD_ERR_INVALID, "dsv_mt_grad_norm: bad max_norm %g (must be >= 0; +inf: no clipping)", max_norm);
    const int64_t need = dsv_mt_workspace_floats(n, count);
    if (workspace_floats < need)
        return fail(DSD_ERR_INVALID, "dsv_mt_grad_norm: the workspace holds %lld floats, dsv_mt_workspace_floats asks for %lld", (long long)workspace_floats, (long long)need);
    MtNormTable tb{};
    auto fill = [&](int slot, int64_t i) { tb.g[slot] = g[i]; tb.n[slot] = n[i]; };
    auto launch = [&](const MtChunks& c, int nc, int64_t first) -> int {
        tb.c = c;
        tb.first_chunk = first;
        hipLaunchKernelGGL(k_mt_norm_partial, dim3((unsigned)nc), dim3(kMtThreads), 0, (hipStream_t)stream, tb, (double*)workspace);
        HIP_TRY(hipGetLastError());
        return DSD_OK;
    };
    DSD_TRY(mt_split(n, count, fill, launch));
    hipLaunchKernelGGL(k_mt_norm_final, dim3(1), dim3(kMtThreads), 0, (hipStream_t)stream, (const double*)workspace, (long long)(need / 2), (float)max_norm, out2);
    HIP_TRY(hipGetLastError());
    return DSD_OK;
}

static int mt_check_step(const char* who, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count,
                         double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* gscale) {
    DSD_TRY(mt_check_counts(who, n, count));
    DSD_TRY(mt_check_pointers(who, "p", (const void* const*)p, count));
    DSD_TRY(mt_check_pointers(who, "g", (const void* const*)g, count));
    DSD_TRY(mt_check_pointers(who, "m", (const void* const*)m, count));
    DSD_TRY(mt_check_pointers(who, "v", (const void* const*)v, count));
    if (step < 1) return fail(DSD_ERR_INVALID, "%s: bad argument (step=%lld must be >= 1)", who, (long long)step);
    if ((uintptr_t)gscale & 3) return fail(DSD_ERR_INVALID, "%s: gscale is not aligned to a float", who);
    if (!(lr >= 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(eps >= 0) || !(weight_decay >= 0))
        return fail(DSD_ERR_INVALID, "%s: bad hyper-parameters (lr=%g betas=%g,%g eps=%g weight_decay=%g)", who, lr, beta1, beta2, eps, weight_decay);
    return DSD_OK;
}

template <class Op>
static int mt_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count, const Op& op, void* stream) {
    MtStepTable tb{};
    auto fill = [&](int slot, int64_t i) { tb.t[slot] = MtTensor{p[i], g[i], m[i], v[i], (long long)n[i]}; };
    auto launch = [&](const MtChunks& c, int nc, int64_t) -> int {
        tb.c = c;
        hipLaunchKernelGGL(k_mt_step<Op>, dim3((unsigned)nc), dim3(kMtThreads), 0, (hipStream_t)stream, tb, op);
        HIP_TRY(hipGetLastError());
        return DSD_OK;
    };
    return mt_split(n, count, fill, launch);
}

// N_sma, step_size and the branch exactly as radam.py:66-76 forms them in double (Python's ** on a float is C's pow)
static void radam_scalars(int64_t step, double beta1, double beta2, double* out3) {
    const double beta2_t = std::pow(beta2, (double)step);
    const double n_sma_max = 2 / (1 - beta2) - 1;
    const double n_sma = n_sma_max - 2 * (double)step * beta2_t / (1 - beta2_t);
    double step_size;
    if (n_sma >= 5)
        step_size = std::sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) / (1 - std::pow(beta1, (double)step));
    else
        step_size = 1.0 / (1 - std::pow(beta1, (double)step));
    out3[0] = n_sma; out3[1] = step_size; out3[2] = n_sma >= 5 ? 1.0 : 0.0;
}

extern "C" int dsv_radam_scalars(int64_t step, double beta1, double beta2, double* out3) {
    if (!out3 || step < 1 || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1))
        return fail(DSD_ERR_INVALID, "dsv_radam_scalars: bad argument (step=%lld >= 1, betas=%g,%g in [0, 1))", (long long)step, beta1, beta2);
    radam_scalars(step, beta1, beta2, out3);
    return DSD_OK;
}

extern "C" int dsv_mt_radam_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* gscale, void* stream) {
    DSD_TRY(mt_check_step("dsv_mt_radam_step", p, g, m, v, n, count, lr, beta1, beta2, eps, weight_decay, step, gscale));
    double sc[3];
    radam_scalars(step, beta1, beta2, sc);
    MtRAdam op{};
    op.gscale = gscale;
    // the Python floats the reference hands to its float32 tensor ops
    op.b1 = (float)beta1; op.one_minus_b1 = (float)(1 - beta1);
    op.b2 = (float)beta2; op.one_minus_b2 = (float)(1 - beta2);
    op.neg_wd_lr = (float)(-weight_decay * lr);
    op.neg_step_lr = (float)(-sc[1] * lr);
    op.eps = (float)eps;
    op.decay = weight_decay != 0;
    op.rectified = sc[2] != 0;
    return mt_step(p, g, m, v, n, count, op, stream);
}

extern "C" int dsv_mt_adamw_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int64_t count, double lr,
                                 double beta1, double beta2, double eps, double weight_decay, int64_t step, const float* gscale, void* stream) {
    DSD_TRY(mt_check_step("dsv_mt_adamw_step", p, g, m, v, n, count, lr, beta1, beta2, eps, weight_decay, step, gscale));
    MtAdamW op{};
    op.gscale = gscale;
    // the scalars as dsf_adamw_step forms them (torch.optim.AdamW's, in double)
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    op.a.decay = (float)(1.0 - lr * weight_decay);
    op.a.one_minus_b1 = (float)(1.0 - beta1);
    op.a.b2 = (float)beta2;
    op.a.one_minus_b2 = (float)(1.0 - beta2);
    op.a.bc2_sqrt = (float)std::sqrt(bc2);
    op.a.eps = (float)eps;
    op.a.neg_step_size = (float)(-(lr / bc1));
    return mt_step(p, g, m, v, n, count, op, stream);
}
