// nd_report.hip -- the tail of a run: row softmax of the conditions (nd_softmax_rows), ensemble aggregation (nd_aggregate), per-sample
// statistics (nd_sample_stats) and the reported numbers (nd_report).  gfx950 only.  Small fixed-order kernels: reproducible sums.
#include "nd_host.hpp"

// ---- softmax over the class dim (classification_train_separately.py:755-758) -----------------
__global__ void k_softmax_rows(const float* __restrict__ x, float* __restrict__ out, int rows, int C) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* p = x + (size_t)r * C;
    float mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(p[c] - mx);
    for (int c = 0; c < C; ++c) out[(size_t)r * C + c] = expf(p[c] - mx) / s;
}

extern "C" int nd_softmax_rows(const float* x, float* out, int rows, int C, void* stream) {
    if (!x || !out) return nd_set_err(ND_ERR_ARG, "softmax: NULL tensor");
    if (rows < 1 || C < 1) return nd_set_err(ND_ERR_ARG, "softmax needs rows, C >= 1 (rows=%d, C=%d)", rows, C);
    hipLaunchKernelGGL(k_softmax_rows, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, x, out, rows, C);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

// ---- aggregation (classification_train_separately.py:51-68, 392-398, 425-447) ------------------
// One thread per image b: loops the S samples in order (member-major then trial), so the mean is a
// fixed-order sum.  convert_to_prob: softmax(-(y-1)^2 / temperature); vote: mode of argmax over the
// raw y_0 (first maximum = smallest label on ties, as torch.argmax / torch.unique+counts.argmax; a NaN counts as the
// maximum and the first NaN is taken, as torch.argmax does).  A NaN or an all-(-inf) logit row gives NaN probabilities
// for that sample and so for the image's mean, as torch.softmax does.
#define ND_AGG_MAX_C 16
__global__ void k_aggregate(const float* __restrict__ samples, float* __restrict__ prob, long long* __restrict__ vote,
                            float* __restrict__ probs, int S, int B, int C, float temperature) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float acc[ND_AGG_MAX_C];
    int cnt[ND_AGG_MAX_C];
    for (int c = 0; c < C; ++c) { acc[c] = 0.f; cnt[c] = 0; }
    for (int s = 0; s < S; ++s) {
        const float* y = samples + ((size_t)s * B + b) * C;
        float lg[ND_AGG_MAX_C];
        int am = 0;
        float best = y[0];
        for (int c = 0; c < C; ++c) {
            const float d = y[c] - 1.0f;
            lg[c] = d * d * (-1.0f) / temperature;
            if (y[c] > best || (y[c] != y[c] && best == best)) { best = y[c]; am = c; }
        }
        cnt[am]++;
        float mx = lg[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg[c]);
        float sum = 0.f;
        for (int c = 0; c < C; ++c) { lg[c] = expf(lg[c] - mx); sum += lg[c]; }
        for (int c = 0; c < C; ++c) {
            const float p = lg[c] / sum;
            acc[c] += p;
            if (probs) probs[((size_t)s * B + b) * C + c] = p;
        }
    }
    int vm = 0;
    for (int c = 1; c < C; ++c) if (cnt[c] > cnt[vm]) vm = c;
    vote[b] = vm;
    for (int c = 0; c < C; ++c) prob[(size_t)b * C + c] = acc[c] / (float)S;
}

extern "C" int nd_aggregate(const float* samples, float* prob_out, int64_t* vote_out, float* probs_out, int S, int B, int C,
                            float temperature, void* stream) {
    if (!samples || !prob_out || !vote_out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (S < 1 || B < 1 || C < 1 || C > ND_AGG_MAX_C) return nd_set_err(ND_ERR_ARG, "S,B >= 1 and 1 <= C <= %d required (S=%d, B=%d, C=%d)", ND_AGG_MAX_C, S, B, C);
    if (!(temperature > 0.f)) return nd_set_err(ND_ERR_ARG, "temperature must be > 0 (temperature=%g)", (double)temperature);
    hipLaunchKernelGGL(k_aggregate, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, samples, prob_out, (long long*)vote_out,
                       probs_out, S, B, C, temperature);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}


// ---- reporting tail (classification_train_separately.py:102-174, 413-423, 801-815) ---------------
// One wave per (image, class): the S per-sample values go to LDS; every lane ranks its elements by counting
// (stable: ties broken by index), the four order statistics needed by the two interpolated quantiles are
// picked by rank.  Variance: two-pass (mean, then centred squares), unbiased.  A NaN among the S values has no rank (it
// compares false with everything), so the picks are not all written: such a (b, c) gets NaN PIW, as torch.quantile
// gives, and pick[] is not read; its variance is NaN through the sums.
#define ND_STATS_MAXS 4096
__global__ __launch_bounds__(64) void k_sample_stats(const float* __restrict__ probs, float* __restrict__ piw, float* __restrict__ var,
                                                     int S, int B, int C, float q_lo, float q_hi) {
#pragma clang fp contract(off)
    const int bc = blockIdx.x, lane = threadIdx.x;
    __shared__ float v[ND_STATS_MAXS];
    __shared__ float pick[4];
    for (int s = lane; s < S; s += 64) v[s] = probs[(size_t)s * B * C + bc];
    __syncthreads();
    const float r_lo = q_lo * (float)(S - 1), r_hi = q_hi * (float)(S - 1);
    const int k0 = (int)floorf(r_lo), k2 = (int)floorf(r_hi);
    const int k1 = min(k0 + 1, S - 1), k3 = min(k2 + 1, S - 1);
    float sum = 0.f;
    int has_nan = 0;
    for (int i = lane; i < S; i += 64) {
        const float vi = v[i];
        sum += vi;
        has_nan |= vi != vi;
        int rank = 0;
        for (int j = 0; j < S; ++j) rank += (v[j] < vi) || (v[j] == vi && j < i);
        if (rank == k0) pick[0] = vi;
        if (rank == k1) pick[1] = vi;
        if (rank == k2) pick[2] = vi;
        if (rank == k3) pick[3] = vi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sum += __shfl_xor(sum, off, 64); has_nan |= __shfl_xor(has_nan, off, 64); }
    const float mean = sum / (float)S;
    float sq = 0.f;
    for (int i = lane; i < S; i += 64) { const float d = v[i] - mean; sq += d * d; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    __syncthreads();
    if (lane == 0) {
        var[bc] = S > 1 ? sq / (float)(S - 1) : NAN;
        if (has_nan) { piw[bc] = NAN; return; }
        // torch.lerp(a, b, w): a + w*(b-a) for w < 0.5, else b - (b-a)*(1-w)
        const float w_lo = r_lo - (float)k0, w_hi = r_hi - (float)k2;
        const float lo = w_lo < 0.5f ? pick[0] + w_lo * (pick[1] - pick[0]) : pick[1] - (pick[1] - pick[0]) * (1.0f - w_lo);
        const float hi = w_hi < 0.5f ? pick[2] + w_hi * (pick[3] - pick[2]) : pick[3] - (pick[3] - pick[2]) * (1.0f - w_hi);
        piw[bc] = hi - lo;
    }
}

extern "C" int nd_sample_stats(const float* probs, float* piw, float* var, int S, int B, int C, float q_lo, float q_hi, void* stream) {
    if (!probs || !piw || !var) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (S < 1 || S > ND_STATS_MAXS || B < 1 || C < 1) return nd_set_err(ND_ERR_ARG, "need 1 <= S <= %d, B,C >= 1 (S=%d, B=%d, C=%d)", ND_STATS_MAXS, S, B, C);
    if (!(q_lo >= 0.f && q_lo <= q_hi && q_hi <= 1.f))
        return nd_set_err(ND_ERR_ARG, "need 0 <= q_lo <= q_hi <= 1 (q_lo=%g, q_hi=%g)", (double)q_lo, (double)q_hi);
    hipLaunchKernelGGL(k_sample_stats, dim3(B * C), dim3(64), 0, (hipStream_t)stream, probs, piw, var, S, B, C, q_lo, q_hi);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}

// One thread per reported number, each a fixed-order loop over the N images (reproducible; N is a test-set size).
#define ND_REPORT_MAXBINS 64
__global__ __launch_bounds__(256) void k_report(const float* __restrict__ piw, const float* __restrict__ var, const float* __restrict__ pm,
                                                const long long* __restrict__ vote, const long long* __restrict__ target,
                                                float* __restrict__ out, int N, int C, float temperature, int n_bins) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __shared__ float ece_part[ND_REPORT_MAXBINS];
    if (tid == 0) {                                         // accuracy
        int correct = 0;
        for (int i = 0; i < N; ++i) correct += vote[i] == target[i];
        out[0] = (float)correct / (float)N;
    }
    if (tid >= 1 && tid <= n_bins) {                        // calibration bin tid-1: (b[k], b[k+1]]
        const int k = tid - 1, steps = n_bins + 1;
        const float step = 1.0f / (float)n_bins;
        auto bound = [&](int i) { return i < steps / 2 ? step * (float)i : 1.0f - step * (float)(steps - 1 - i); };   // torch.linspace
        const float lo = bound(k), hi = bound(k + 1);
        float cnt = 0.f, csum = 0.f, asum = 0.f;
        for (int i = 0; i < N; ++i) {
            // convert_to_prob on the averaged probabilities (quirk kept), then confidence = max, prediction = argmax
            float mx = -INFINITY, lg[16];
            for (int c = 0; c < C; ++c) { const float d = pm[(size_t)i * C + c] - 1.0f; lg[c] = d * d * (-1.0f) / temperature; mx = fmaxf(mx, lg[c]); }
            float sum = 0.f;
            for (int c = 0; c < C; ++c) { lg[c] = expf(lg[c] - mx); sum += lg[c]; }
            float conf = -1.f; int pred = 0;
            for (int c = 0; c < C; ++c) { const float pc = lg[c] / sum; if (pc > conf) { conf = pc; pred = c; } }
            if (conf > lo && conf <= hi) { cnt += 1.f; csum += conf; asum += (pred == (int)target[i]) ? 1.f : 0.f; }
        }
        ece_part[k] = cnt > 0.f ? fabsf(asum / cnt - csum / cnt) * (cnt / (float)N) : 0.f;
    }
    const int q = tid - 128;                                // class statistics: q = kind * C + c
    if (q >= 0 && q < 4 * C) {
        const int kind = q / C, c = q % C;                  // 0 piw correct, 1 piw incorrect, 2 var correct, 3 var incorrect
        float sum = 0.f; int cnt = 0;
        for (int i = 0; i < N; ++i) {
            const int mv = (int)vote[i], gt = (int)target[i];
            if (mv != c) continue;
            const bool correct = mv == gt;
            if ((kind & 1) == (correct ? 0 : 1)) {
                sum += kind < 2 ? piw[(size_t)i * C + mv] : var[(size_t)i * C + c];
                ++cnt;
            }
        }
        out[2 + q] = kind < 2 ? sum / (float)cnt : (cnt > 0 ? sum / (float)cnt : 0.f);   // empty: NaN for PIW, 0 for variance
    }
    __syncthreads();
    if (tid == 0) {
        float e = 0.f;
        for (int k = 0; k < n_bins; ++k) e += ece_part[k];
        out[1] = e;
    }
}

extern "C" int nd_report(const float* piw, const float* var, const float* pm, const int64_t* vote, const int64_t* target, float* out,
                         int N, int C, float temperature, int n_bins, void* stream) {
    if (!piw || !var || !pm || !vote || !target || !out) return nd_set_err(ND_ERR_ARG, "NULL tensor");
    if (N < 1 || C < 1 || C > 16 || n_bins < 1 || n_bins > ND_REPORT_MAXBINS) return nd_set_err(ND_ERR_ARG, "need N >= 1, 1 <= C <= 16, 1 <= n_bins <= %d (N=%d, C=%d, n_bins=%d)", ND_REPORT_MAXBINS, N, C, n_bins);
    if (!(temperature > 0.f)) return nd_set_err(ND_ERR_ARG, "temperature must be > 0 (temperature=%g)", (double)temperature);
    hipLaunchKernelGGL(k_report, dim3(1), dim3(256), 0, (hipStream_t)stream, piw, var, pm, (const long long*)vote, (const long long*)target, out,
                       N, C, temperature, n_bins);
    HIP_CHECK(hipGetLastError());
    return ND_OK;
}
