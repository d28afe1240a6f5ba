// dvdr_periodic_kernels.hip -- the line-of-sight velocity-gradient correction of a coeval box with a
// PERIODIC line of sight (reference: src/py21cmfast/rsds.py:16-103, include_dvdr_in_tau21 with
// periodic = True, as Coeval.include_dvdr_in_tau21 calls it, drivers/coeval.py:242-278).
//
// The reference's gradient is irfftn(1j k_z rfftn(v)): only k_z enters, the x and y transforms cancel,
// and what is left is the spectral derivative of every z-line, g = irfft(i k rfft(v)) with
// k = 2 pi rfftfreq(n, dx).  z is the fastest axis (float[n_cols][n]), so one launch reads v, T_b (and
// tau_21), differentiates the lines in LDS and registers and writes the corrected T_b: 12 B per cell,
// 16 B with tau_21; no spectrum ever reaches HBM.
//
// Two paths:
//   transform (n = 2^k, 8 <= n <= 1024): the derivative is a real circulant matrix, so applied to
//     a + i b it gives a' + i b': two real lines travel as one complex line with no r2c untangling.
//     n = A B; forward: DFT_A over a of x[B a + b], twiddle W_n^(b k1), DFT_B over b -> X[k1 + A k2];
//     times i k_signed / n (fftfreq with the Nyquist entry 0); the inverse runs the same two steps
//     backwards, so the DFT_B pair and the multiplication stay in the registers of one lane.  fp32, the
//     butterflies of fft_device.h.  A workgroup owns a batch of line pairs; a pair's n points live in
//     LDS as A rows of B + 1 float2 (the pad keeps both the column and the row accesses conflict-free).
//   direct (every other n from 2 to 1536, any n when forced): the exact circulant sum
//     g_j = sum_m d[(j - m) mod n] v_m in fp64, d_0 = 0,
//     d_j = (2 pi / (n dx)) (1/2) (-1)^j cot(pi j / n)  (n even),  ... / sin(pi j / n)  (n odd).
//     The table is built once per workgroup in fp64 (d_(n-j) = -d_j taken from the lower half, so a
//     constant and a Nyquist line cancel term by term), stored twice over so that no index wraps; a
//     lane owns four consecutive cells of a line and slides a four-entry window over the table: two
//     LDS reads per four multiply-adds.  The gradient is rounded to fp32 once, into LDS, for the
//     coalesced epilogue.
// The epilogue of both is the per-cell arithmetic of lightcone_dvdr_kernel, term for term.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
#include "fft_device.h"

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 8;
constexpr int kDirectMaxN = 1536;
constexpr int kDirectCells = 3072;  // floats of one direct batch: two lines of 1536

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                       \
            return C21CM_IO_ERROR;                                                      \
        }                                                                               \
    } while (0)

struct DvdrArgs {
    float *out;
    const float *bt;
    const float *vel;
    const float *tau;
    const double *hubble;
    size_t n_cols;
    int n;
    double dx;
    double max_dvdr;
    int use_ts;
    int vec;  // every array pointer is 16-byte aligned: float4 accesses where the offset allows
};

// rsds.py:81-101 on one cell, as lightcone_dvdr_kernel does it
__device__ __forceinline__ float corrected(float bt, float grad_f, double H, double max_dvdr, int use_ts,
                                           float tau) {
    const double grad = (double)grad_f;
    if (!use_ts) {
        const double mx = max_dvdr * H;
        const double d = grad < -mx ? -mx : (grad > mx ? mx : grad);
        return (float)((double)bt / fabs(1.0 + d / H));
    }
    const double ta = (double)tau;
    const double g = fabs(1.0 + grad / H);
    double fac = (1.0 - exp(-ta / g)) / (1.0 - exp(-ta));
    if (ta < 1e-10) fac = 1.0;
    return bt * (float)fac;
}

// A batch is `cnt` consecutive floats of every array from element `off` on, whole lines of n cells.
// Split it into a scalar head up to the first 16-byte boundary, float4 groups and a scalar tail.
__device__ __forceinline__ void split(const DvdrArgs &p, size_t off, int cnt, int &head, int &nvec) {
    head = p.vec ? (int)((4 - (off & 3)) & 3) : cnt;
    if (head > cnt) head = cnt;
    nvec = (cnt - head) / 4;
}

// out = corrected(bt) for the batch; grad(i): the gradient of cell i of the batch (from LDS)
template <class Grad>
__device__ __forceinline__ void epilogue(const DvdrArgs &p, size_t off, int cnt, const double *hs, Grad grad) {
    int head, nvec;
    split(p, off, cnt, head, nvec);
    const int n = p.n;
    const float *bt = p.bt + off, *tau = p.use_ts ? p.tau + off : nullptr;
    float *out = p.out + off;
    for (int t = threadIdx.x; t < nvec; t += kBlock) {
        const int i = head + 4 * t;
        const float4 b = *reinterpret_cast<const float4 *>(bt + i);
        float4 ta = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.use_ts) ta = *reinterpret_cast<const float4 *>(tau + i);
        const float bb[4] = {b.x, b.y, b.z, b.w}, tt[4] = {ta.x, ta.y, ta.z, ta.w};
        float r[4];
        int k = i % n;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = corrected(bb[j], grad(i + j), hs[k], p.max_dvdr, p.use_ts, tt[j]);
            if (++k == n) k = 0;
        }
        *reinterpret_cast<float4 *>(out + i) = make_float4(r[0], r[1], r[2], r[3]);
    }
    const int tail0 = head + 4 * nvec;
    for (int t = threadIdx.x; t < head + (cnt - tail0); t += kBlock) {
        const int i = t < head ? t : tail0 + (t - head);
        out[i] = corrected(bt[i], grad(i), hs[i % n], p.max_dvdr, p.use_ts, p.use_ts ? tau[i] : 0.f);
    }
}

// ------------------------------------------------------------------ transform path
template <int A, int B>
struct FftShape {
    static constexpr int N = A * B;
    static constexpr int LP = A * (B + 1);  // float2 per complex line in LDS
    static constexpr int kMinAB = A < B ? A : B;
    static constexpr int kWant = kBlock / kMinAB;              // every lane busy in the narrower pass
    static constexpr int kFit = (40 * 1024) / (LP * 8);        // lines within 40 KB
    static constexpr int LINES = kWant < kFit ? kWant : (kFit < 1 ? 1 : kFit);
};

template <int A, int B>
__global__ void __launch_bounds__(kBlock)
dvdr_periodic_fft_kernel(DvdrArgs p, double kscale, size_t n_batches) {
    using Sh = FftShape<A, B>;
    constexpr int N = Sh::N, LP = Sh::LP, LINES = Sh::LINES;
    __shared__ float2 L[LINES * LP];
    __shared__ float2 TW[LP];  // TW[k1 (B + 1) + b] = exp(-2 pi i b k1 / N)
    __shared__ double HS[N];
    float *Lf = reinterpret_cast<float *>(L);
    const int tid = threadIdx.x;

    for (int t = tid; t < A * B; t += kBlock) {
        const int k1 = t / B, b = t % B;
        double s, c;
        sincospi(-2.0 * (double)(b * k1) / (double)N, &s, &c);
        TW[k1 * (B + 1) + b] = make_float2((float)c, (float)s);
    }
    for (int t = tid; t < N; t += kBlock) HS[t] = p.hubble[t];

    // float index of point n of real line r (of the batch) in L: pair r / 2, component r % 2
    auto slot = [](int r, int n) { return 2 * ((r >> 1) * LP + (n / B) * (B + 1) + (n % B)) + (r & 1); };

    for (size_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const size_t line0 = batch * (size_t)(2 * LINES);
        const size_t left = p.n_cols - line0;
        const int lines = left < (size_t)(2 * LINES) ? (int)left : 2 * LINES;  // real lines of this batch
        const int pairs = (lines + 1) / 2;
        const size_t off = line0 * (size_t)N;
        const int cnt = lines * N;
        __syncthreads();  // the last batch's epilogue has read L; the tables are written
        {
            int head, nvec;
            split(p, off, cnt, head, nvec);  // N is a multiple of 4: head is 0 or cnt
            const float *v = p.vel + off;
            for (int t = tid; t < nvec; t += kBlock) {
                const int i = head + 4 * t;
                const float4 x = *reinterpret_cast<const float4 *>(v + i);
                const int r = i / N, n = i % N;
                Lf[slot(r, n)] = x.x;
                Lf[slot(r, n + 1)] = x.y;
                Lf[slot(r, n + 2)] = x.z;
                Lf[slot(r, n + 3)] = x.w;
            }
            for (int i = tid; i < head; i += kBlock) Lf[slot(i / N, i % N)] = v[i];
            if (lines & 1)  // the unpaired line: a zero imaginary part
                for (int n = tid; n < N; n += kBlock) Lf[slot(lines, n)] = 0.f;
        }
        __syncthreads();
        // forward step 1: DFT_A down column b, times W_N^(b k1)
        for (int w = tid; w < pairs * B; w += kBlock) {
            float2 *Lq = L + (w / B) * LP;
            const int b = w % B;
            float2 x[A];
#pragma unroll
            for (int a = 0; a < A; ++a) x[a] = Lq[a * (B + 1) + b];
            Dft<A, -1>::run(x);
#pragma unroll
            for (int k1 = 0; k1 < A; ++k1) Lq[k1 * (B + 1) + b] = cmul(x[k1], TW[k1 * (B + 1) + b]);
        }
        __syncthreads();
        // forward step 2 along row k1 -> X[k1 + A k2]; i k X / N; inverse step 1 back into the row
        for (int w = tid; w < pairs * A; w += kBlock) {
            float2 *Lq = L + (w / A) * LP;
            const int k1 = w % A;
            float2 y[B];
#pragma unroll
            for (int b = 0; b < B; ++b) y[b] = Lq[k1 * (B + 1) + b];
            Dft<B, -1>::run(y);
#pragma unroll
            for (int k2 = 0; k2 < B; ++k2) {
                const int k = k1 + A * k2;
                const int ks = 2 * k < N ? k : (2 * k == N ? 0 : k - N);
                const float m = (float)((double)ks * kscale);
                y[k2] = make_float2(-m * y[k2].y, m * y[k2].x);
            }
            Dft<B, +1>::run(y);
#pragma unroll
            for (int b = 0; b < B; ++b) Lq[k1 * (B + 1) + b] = cmulc(y[b], TW[k1 * (B + 1) + b]);
        }
        __syncthreads();
        // inverse step 2: DFT_A up column b -> g[B a + b]
        for (int w = tid; w < pairs * B; w += kBlock) {
            float2 *Lq = L + (w / B) * LP;
            const int b = w % B;
            float2 x[A];
#pragma unroll
            for (int k1 = 0; k1 < A; ++k1) x[k1] = Lq[k1 * (B + 1) + b];
            Dft<A, +1>::run(x);
#pragma unroll
            for (int a = 0; a < A; ++a) Lq[a * (B + 1) + b] = x[a];
        }
        __syncthreads();
        epilogue(p, off, cnt, HS, [&](int i) { return Lf[slot(i / N, i % N)]; });
    }
}

// ------------------------------------------------------------------ direct path
// dynamic LDS: D2[2 n + 4] and HS[n] doubles, then V and G, kDirectCells floats each
inline size_t direct_lds_bytes(int n) {
    return sizeof(double) * (size_t)(3 * n + 4) + 2 * sizeof(float) * (size_t)kDirectCells;
}

__global__ void __launch_bounds__(kBlock)
dvdr_periodic_direct_kernel(DvdrArgs p, int lines_per_batch, size_t n_batches) {
    extern __shared__ double dyn_lds[];
    const int tid = threadIdx.x, n = p.n;
    double *D2 = dyn_lds;                                   // D2[e] = d[e mod n]
    double *HS = D2 + 2 * n + 4;
    float *V = reinterpret_cast<float *>(HS + n);           // the lines of a batch
    float *G = V + kDirectCells;                            // their gradients
    const double c = M_PI / ((double)n * p.dx);  // (2 pi / (n dx)) / 2
    for (int e = tid; e < 2 * n + 4; e += kBlock) {
        const int r = e % n;
        const int j = r <= n - r ? r : n - r;  // d_(n-j) = -d_j: the lower half carries the table
        double d = 0.0;
        if (r != 0 && 2 * r != n) {
            const double x = (double)j / (double)n;
            d = (n & 1) ? c / sinpi(x) : c * cospi(x) / sinpi(x);
            if (j & 1) d = -d;
            if (j != r) d = -d;
        }
        D2[e] = d;
    }
    for (int t = tid; t < n; t += kBlock) HS[t] = p.hubble[t];
    const int groups = (n + 3) / 4;  // four consecutive cells of a line per lane

    for (size_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
        const size_t line0 = batch * (size_t)lines_per_batch;
        const size_t left = p.n_cols - line0;
        const int lines = left < (size_t)lines_per_batch ? (int)left : lines_per_batch;
        const size_t off = line0 * (size_t)n;
        const int cnt = lines * n;
        __syncthreads();  // the last batch's epilogue has read G; the tables are written
        {
            int head, nvec;
            split(p, off, cnt, head, nvec);
            const float *v = p.vel + off;
            for (int t = tid; t < nvec; t += kBlock) {
                const int i = head + 4 * t;
                const float4 x = *reinterpret_cast<const float4 *>(v + i);
                V[i] = x.x, V[i + 1] = x.y, V[i + 2] = x.z, V[i + 3] = x.w;
            }
            const int tail0 = head + 4 * nvec;
            for (int t = tid; t < head + (cnt - tail0); t += kBlock) {
                const int i = t < head ? t : tail0 + (t - head);
                V[i] = v[i];
            }
        }
        __syncthreads();
        const int items = lines * groups;
        for (int w = tid; w < items; w += kBlock) {
            const int l = w / groups, j0 = 4 * (w - l * groups);
            const float *vl = V + l * n;
            const double *dw = D2 + j0 + n;  // dw[r - m] = d[(j0 + r - m) mod n], 0 <= r < 4
            double w0 = dw[0], w1 = dw[1], w2 = dw[2], w3 = dw[3];
            double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
#pragma unroll 4
            for (int m = 0; m < n; ++m) {
                const double vm = (double)vl[m];
                g0 = fma(w0, vm, g0);
                g1 = fma(w1, vm, g1);
                g2 = fma(w2, vm, g2);
                g3 = fma(w3, vm, g3);
                w3 = w2, w2 = w1, w1 = w0;
                w0 = dw[-(m + 1)];  // the last one, D2[j0], is inside the table and not used
            }
            float *gl = G + l * n + j0;
            gl[0] = (float)g0;
            if (j0 + 1 < n) gl[1] = (float)g1;
            if (j0 + 2 < n) gl[2] = (float)g2;
            if (j0 + 3 < n) gl[3] = (float)g3;
        }
        __syncthreads();
        epilogue(p, off, cnt, HS, [&](int i) { return G[i]; });
    }
}
}  // namespace

// k-th supported transform shape: n = A B
#define DVDR_FFT_SHAPES(X) X(4, 2) X(4, 4) X(8, 4) X(8, 8) X(16, 8) X(16, 16) X(32, 16) X(32, 32)

extern "C" int c21hip_dvdr_periodic(float *bt_out, const float *bt_in, const float *vel, const float *tau,
                                    const double *hubble, size_t n_cols, int n, double dx, double max_dvdr,
                                    int use_ts, int method, void *stream) {
    if (!bt_out || !bt_in || !vel || !hubble || (use_ts && !tau)) {
        c21hip_set_error("periodic dvdr: a required array pointer is NULL");
        return C21CM_VALUE_ERROR;
    }
    if (method < 0 || method > 2) {
        c21hip_set_error("periodic dvdr: method %d is not 0 (automatic), 1 (transform) or 2 (direct)", method);
        return C21CM_VALUE_ERROR;
    }
    if (n < 2) {
        c21hip_set_error("periodic dvdr: a line needs at least 2 points, not %d", n);
        return C21CM_VALUE_ERROR;
    }
    if (!(dx > 0.0) || !std::isfinite(dx) || !(max_dvdr >= 0.0) || !std::isfinite(max_dvdr)) {
        c21hip_set_error("periodic dvdr: dx must be positive and max_dvdr >= 0, both finite");
        return C21CM_VALUE_ERROR;
    }
    const bool pow2 = (n & (n - 1)) == 0 && n >= 8 && n <= 1024;
    if (method == 1 && !pow2) {
        c21hip_set_error("periodic dvdr: the transform path takes n = 2^k, 8 <= n <= 1024, not %d", n);
        return C21CM_VALUE_ERROR;
    }
    if (method == 0) method = pow2 ? 1 : 2;
    if (method == 2 && n > kDirectMaxN) {
        c21hip_set_error("periodic dvdr: the direct path takes 2 <= n <= %d, not %d", kDirectMaxN, n);
        return C21CM_VALUE_ERROR;
    }
    if (n_cols == 0) return 0;
    if (n_cols > (size_t)0x7FFFFFFF * 256u) {
        c21hip_set_error("periodic dvdr: too many lines");
        return C21CM_VALUE_ERROR;
    }
    DvdrArgs p{bt_out, bt_in, vel, use_ts ? tau : nullptr, hubble, n_cols, n, dx, max_dvdr, use_ts ? 1 : 0, 0};
    const uintptr_t bits = (uintptr_t)bt_out | (uintptr_t)bt_in | (uintptr_t)vel | (uintptr_t)p.tau;
    p.vec = (bits & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (method == 1) {
        const double kscale = 2.0 * M_PI / ((double)n * dx) / (double)n;
#define LAUNCH_SHAPE(A, B)                                                                              \
    if (n == (A) * (B)) {                                                                               \
        const size_t per = 2 * (size_t)FftShape<A, B>::LINES, nb = (n_cols + per - 1) / per;            \
        const int grid = (int)(nb < (size_t)kMaxBlocks ? nb : (size_t)kMaxBlocks);                      \
        hipLaunchKernelGGL((dvdr_periodic_fft_kernel<A, B>), dim3(grid), dim3(kBlock), 0, st, p, kscale, nb); \
    }
        DVDR_FFT_SHAPES(LAUNCH_SHAPE)
#undef LAUNCH_SHAPE
    } else {
        const int per = kDirectCells / n;  // >= 2: n <= 1536
        const size_t nb = (n_cols + (size_t)per - 1) / (size_t)per;
        const int grid = (int)(nb < (size_t)kMaxBlocks ? nb : (size_t)kMaxBlocks);
        hipLaunchKernelGGL(dvdr_periodic_direct_kernel, dim3(grid), dim3(kBlock), direct_lds_bytes(n), st, p,
                           per, nb);
    }
    LAUNCH_CHECK();
    return 0;
}
