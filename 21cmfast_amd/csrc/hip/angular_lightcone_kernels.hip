// angular_lightcone_kernels.hip -- angular lightcone assembly (reference: src/py21cmfast/lightconers.py
// AngularLightconer :541-701 and make_lightcone_slices :162-287; the interpolation convention of
// cosmotile's make_lightcone_slice_interpolator / make_lightcone_slice_vector_field as DESIGN 4.10
// states it) and the periodic B-spline prefilter of its orders 3 and 5 (scipy.ndimage.spline_filter,
// mode="grid-wrap").
//
// Sampling: pixel p of the slice at comoving distance d [cells] sits at x = d n_p + origin, n_p the
// rotated unit direction.  x is wrapped per axis and the B-spline taps of the order (1, 8, 64 or 216)
// are read from both node boxes; each tap is redshift-interpolated first, (w_lo a + w_hi b) / w_norm in
// fp64 (mean_max: the larger of a and b where the fp32 product a b < 0), then weighted.  The sum is fp64,
// stored as fp32 into float[n_pix][n_slices] (slices fastest).  A vector field (three components)
// stores sum_k n_k v_k(x).  A lane owns one (pixel, slice) cell with consecutive lanes on consecutive
// slices of a pixel, so a workgroup covers 256 / run neighbouring pixels over their whole run: their
// taps are neighbouring cells of the node boxes and share L2 lines.
//
// Prefilter: one lane owns one line of the box along the filtered axis and runs, per pole z, the causal
// and the anticausal recursion, each started from its periodic sum (truncated where |z|^i < 1e-18).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "c21hip.h"
#include "c21cm_abi.h"

namespace {
constexpr int kBlock = 256;
constexpr int kMaxBlocks = 256 * 8;

inline int grid_for(size_t work_items) {
    size_t b = (work_items + kBlock - 1) / kBlock;
    if (b > (size_t)kMaxBlocks) b = kMaxBlocks;
    if (b < 1) b = 1;
    return (int)b;
}

#define LAUNCH_CHECK()                                                                  \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            c21hip_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                       \
            return C21CM_IO_ERROR;                                                      \
        }                                                                               \
    } while (0)

// the box and output pointers of one launch (a kernel argument: uniform, scalar loads)
struct AngFields {
    const float *lo[C21HIP_ANG_MAX_BOXES];
    const float *hi[C21HIP_ANG_MAX_BOXES];
    float *dst[C21HIP_LC_MAX_FIELDS];
    long dst_stride[C21HIP_LC_MAX_FIELDS];
    long dst_off[C21HIP_LC_MAX_FIELDS];
};

// B-spline weights of the ORDER + 1 taps starting at start(x) (scipy's get_spline_interpolation_weights)
template <int ORDER>
__device__ inline long long spline_taps(double x, double *w) {
    if constexpr (ORDER == 0) {
        w[0] = 1.0;
        return (long long)floor(x + 0.5);
    } else {
        const double fl = floor(x);
        const double t = x - fl; // exact
        if constexpr (ORDER == 1) {
            w[0] = 1.0 - t;
            w[1] = t;
            return (long long)fl;
        } else if constexpr (ORDER == 3) {
            const double z = 1.0 - t;
            w[0] = z * z * z / 6.0;
            w[1] = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0;
            w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
            w[3] = t * t * t / 6.0;
            return (long long)fl - 1;
        } else {
            // beta5 at the distances t + 2, t + 1, t, 1 - t, 2 - t, 3 - t
            auto inner = [](double a) { // |a| < 1
                const double a2 = a * a;
                return 11.0 / 20.0 - a2 / 2.0 + a2 * a2 / 4.0 - a2 * a2 * a / 12.0;
            };
            auto middle = [](double a) { // 1 <= a < 2
                const double a2 = a * a;
                return 17.0 / 40.0 + 5.0 / 8.0 * a - 7.0 / 4.0 * a2 + 5.0 / 4.0 * a2 * a - 3.0 / 8.0 * a2 * a2 +
                       a2 * a2 * a / 24.0;
            };
            auto outer = [](double a) { // 2 <= a < 3
                const double b = 3.0 - a, b2 = b * b;
                return b2 * b2 * b / 120.0;
            };
            const double u = 1.0 - t;
            w[0] = outer(t + 2.0);
            w[1] = middle(t + 1.0);
            w[2] = inner(t);
            w[3] = inner(u);
            w[4] = middle(u + 1.0);
            w[5] = outer(u + 2.0);
            return (long long)fl - 2;
        }
    }
}

template <int ORDER>
__device__ inline void axis_taps(double x, int n, double *w, int *idx) {
    constexpr int T = ORDER + 1;
    const long long s = spline_taps<ORDER>(x, w);
    int m = (int)(s % n);
    if (m < 0) m += n;
#pragma unroll
    for (int a = 0; a < T; ++a) {
        idx[a] = m;
        if (++m == n) m = 0;
    }
}

template <int ORDER, typename Index>
__global__ void __launch_bounds__(kBlock)
angular_sample_kernel(AngFields f, int n_fields, unsigned mean_max, unsigned vec, Index n_pix, Index run,
                      int n0, int n1, int n2, const double *__restrict__ nhat, double ox, double oy,
                      double oz, const c21hip_ang_slice *__restrict__ tab, double w_norm, int *__restrict__ bad) {
    constexpr int T = ORDER + 1;
    const Index total = n_pix * run;
    int flag = 0;
    for (Index t = (Index)blockIdx.x * kBlock + threadIdx.x; t < total; t += (Index)gridDim.x * kBlock) {
        const Index pix = t / run;
        const Index j = t - pix * run;
        const c21hip_ang_slice s = tab[j];
        const double nx = nhat[pix], ny = nhat[(size_t)n_pix + pix], nz = nhat[2 * (size_t)n_pix + pix];
        // x = d n + origin, rounded as numpy rounds it (the library builds with -ffp-contract=off)
        double wx[T], wy[T], wz[T];
        int ix[T], iy[T], iz[T];
        axis_taps<ORDER>(s.d * nx + ox, n0, wx, ix);
        axis_taps<ORDER>(s.d * ny + oy, n1, wy, iy);
        axis_taps<ORDER>(s.d * nz + oz, n2, wz, iz);
        int b = 0;
        for (int q = 0; q < n_fields; ++q) {
            const int ncomp = ((vec >> q) & 1u) ? 3 : 1;
            const bool mm = (mean_max >> q) & 1u;
            double comp[3] = {0.0, 0.0, 0.0};
            for (int c = 0; c < ncomp; ++c, ++b) {
                const float *__restrict__ lo = f.lo[b];
                const float *__restrict__ hi = f.hi[b];
                double acc = 0.0;
#pragma unroll
                for (int a0 = 0; a0 < T; ++a0) {
#pragma unroll
                    for (int a1 = 0; a1 < T; ++a1) {
                        const double w01 = wx[a0] * wy[a1];
                        const size_t row = ((size_t)ix[a0] * (size_t)n1 + (size_t)iy[a1]) * (size_t)n2;
#pragma unroll
                        for (int a2 = 0; a2 < T; ++a2) {
                            const float va = lo[row + iz[a2]];
                            const float vb = hi[row + iz[a2]];
                            double v = (s.w_lo * (double)va + s.w_hi * (double)vb) / w_norm;
                            if (mm && va * vb < 0.0f) v = (double)(va > vb ? va : vb);
                            acc += (w01 * wz[a2]) * v;
                        }
                    }
                }
                comp[c] = acc;
            }
            const double out = ncomp == 3 ? comp[0] * nx + comp[1] * ny + comp[2] * nz : comp[0];
            flag |= !isfinite(out); // a non-finite tap makes its sum non-finite (0 * inf is NaN)
            f.dst[q][(size_t)pix * (size_t)f.dst_stride[q] + (size_t)f.dst_off[q] + (size_t)j] = (float)out;
        }
    }
    if (flag) atomicOr(bad, 1);
}

// one pole of the periodic prefilter on the line at p[0], p[stride], ... (length L): src -> dst in
// place or not (a lane reads every element of its line before it writes it)
__device__ inline void prefilter_pole(const float *src, float *dst, size_t stride, int L, double z) {
    const double lam = (1.0 - z) * (1.0 - 1.0 / z);
    // |z|^h < 1e-18: the periodic sums end there (the full period when the line is shorter)
    const int horizon = (int)ceil(-18.0 * 2.302585092994046 / log(fabs(z)));
    const int h = L < horizon ? L : horizon;
    const double zL = L < horizon ? pow(z, (double)L) : 0.0;
    // causal: c+[0] = lam sum_i z^i s[-i mod L] / (1 - z^L)
    double sum = 0.0, zi = 1.0;
    for (int i = 0; i < h; ++i) {
        const int k = i == 0 ? 0 : L - i;
        sum += zi * (double)src[(size_t)k * stride];
        zi *= z;
    }
    double c = lam * sum / (1.0 - zL);
    dst[0] = (float)c;
    for (int k = 1; k < L; ++k) {
        c = lam * (double)src[(size_t)k * stride] + z * c;
        dst[(size_t)k * stride] = (float)c;
    }
    // anticausal: c-[L-1] = -z / (1 - z^L) sum_i z^i c+[(L - 1 + i) mod L]
    sum = 0.0;
    zi = 1.0;
    for (int i = 0; i < h; ++i) {
        const int k = i == 0 ? L - 1 : i - 1;
        sum += zi * (double)dst[(size_t)k * stride];
        zi *= z;
    }
    c = -z * sum / (1.0 - zL);
    dst[(size_t)(L - 1) * stride] = (float)c;
    for (int k = L - 2; k >= 0; --k) {
        c = z * (c - (double)dst[(size_t)k * stride]);
        dst[(size_t)k * stride] = (float)c;
    }
}

__global__ void __launch_bounds__(kBlock)
prefilter_axis_kernel(const float *src, float *dst, size_t n_lines, int L, size_t inner, int n_poles,
                      double z1, double z2, int check, int *__restrict__ bad) {
    int flag = 0;
    for (size_t line = (size_t)blockIdx.x * kBlock + threadIdx.x; line < n_lines;
         line += (size_t)gridDim.x * kBlock) {
        const size_t o = line / inner, r = line - o * inner;
        const size_t base = o * (size_t)L * inner + r;
        if (check)
            for (int k = 0; k < L; ++k) flag |= !isfinite(src[base + (size_t)k * inner]);
        prefilter_pole(src + base, dst + base, inner, L, z1);
        if (n_poles > 1) prefilter_pole(dst + base, dst + base, inner, L, z2);
    }
    if (flag) atomicOr(bad, 1);
}

template <int ORDER>
void launch_sample(const AngFields &f, int n_fields, unsigned mean_max, unsigned vec, size_t n_pix, int run,
                   int n0, int n1, int n2, const double *nhat, const double *origin, const c21hip_ang_slice *tab,
                   double w_norm, int *bad, hipStream_t st) {
    const size_t total = n_pix * (size_t)run;
    if (total <= 0xFFFFFFFFull - (size_t)kBlock * kMaxBlocks) { // 32-bit index: cheap pixel divide
        hipLaunchKernelGGL((angular_sample_kernel<ORDER, uint32_t>), dim3(grid_for(total)), dim3(kBlock), 0, st,
                           f, n_fields, mean_max, vec, (uint32_t)n_pix, (uint32_t)run, n0, n1, n2, nhat,
                           origin[0], origin[1], origin[2], tab, w_norm, bad);
    } else {
        hipLaunchKernelGGL((angular_sample_kernel<ORDER, size_t>), dim3(grid_for(total)), dim3(kBlock), 0, st,
                           f, n_fields, mean_max, vec, n_pix, (size_t)run, n0, n1, n2, nhat, origin[0],
                           origin[1], origin[2], tab, w_norm, bad);
    }
}
}  // namespace

extern "C" int c21hip_angular_sample(const float *const *lo, const float *const *hi, float *const *dst,
                                     const long *dst_stride, const long *dst_off, int n_fields,
                                     unsigned mean_max, unsigned vec, int order, size_t n_pix, int run,
                                     int n0, int n1, int n2, const double *nhat, const double *origin,
                                     const c21hip_ang_slice *tab, double w_norm, int *bad, void *stream) {
    if (n_fields < 1 || n_fields > C21HIP_LC_MAX_FIELDS || run < 1 || n0 < 1 || n1 < 1 || n2 < 1 ||
        (order != 0 && order != 1 && order != 3 && order != 5)) {
        c21hip_set_error("angular lightcone: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    AngFields f{};
    int b = 0;
    for (int q = 0; q < n_fields; ++q) {
        const int ncomp = ((vec >> q) & 1u) ? 3 : 1;
        for (int c = 0; c < ncomp; ++c, ++b) {
            f.lo[b] = lo[b];
            f.hi[b] = hi[b];
        }
        f.dst[q] = dst[q];
        f.dst_stride[q] = dst_stride[q];
        f.dst_off[q] = dst_off[q];
        if (dst_off[q] < 0 || dst_off[q] + run > dst_stride[q]) {
            c21hip_set_error("angular lightcone: bad output stride");
            return C21CM_VALUE_ERROR;
        }
    }
    if (n_pix == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    switch (order) {
    case 0: launch_sample<0>(f, n_fields, mean_max, vec, n_pix, run, n0, n1, n2, nhat, origin, tab, w_norm, bad, st); break;
    case 1: launch_sample<1>(f, n_fields, mean_max, vec, n_pix, run, n0, n1, n2, nhat, origin, tab, w_norm, bad, st); break;
    case 3: launch_sample<3>(f, n_fields, mean_max, vec, n_pix, run, n0, n1, n2, nhat, origin, tab, w_norm, bad, st); break;
    default: launch_sample<5>(f, n_fields, mean_max, vec, n_pix, run, n0, n1, n2, nhat, origin, tab, w_norm, bad, st); break;
    }
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_spline_prefilter(const float *src, float *dst, int n0, int n1, int n2, int order, int *bad,
                                       void *stream) {
    if (n0 < 1 || n1 < 1 || n2 < 1 || (order != 3 && order != 5)) {
        c21hip_set_error("spline prefilter: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const double z1 = order == 3 ? sqrt(3.0) - 2.0 : -0.4305753470999737;
    const double z2 = order == 3 ? 0.0 : -0.04309628820326465;
    const int n_poles = order == 3 ? 1 : 2;
    const int dims[3] = {n0, n1, n2};
    const size_t total = (size_t)n0 * n1 * n2;
    for (int axis = 0; axis < 3; ++axis) {
        const int L = dims[axis];
        size_t inner = 1;
        for (int a = axis + 1; a < 3; ++a) inner *= (size_t)dims[a];
        const size_t n_lines = total / (size_t)L;
        hipLaunchKernelGGL(prefilter_axis_kernel, dim3(grid_for(n_lines)), dim3(kBlock), 0, (hipStream_t)stream,
                           axis == 0 ? src : dst, dst, n_lines, L, inner, n_poles, z1, z2, axis == 0, bad);
        LAUNCH_CHECK();
    }
    return 0;
}
