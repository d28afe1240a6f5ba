// lightcone_kernels.hip -- rectilinear lightcone assembly (reference: src/py21cmfast/lightconers.py
// make_lightcone_slices :162-287, RectilinearLightconer.coeval_subselect :505-515,
// redshift_interpolation :295-319) and the line-of-sight velocity-gradient correction of the
// brightness temperature (rsds.py:16-103, include_dvdr_in_tau21 with periodic = False).
//
// Layouts: node boxes float[HII_DIM][HII_DIM][HII_D_PARA], lightcone float[HII_DIM][HII_DIM][n_slices];
// the line of sight is the fastest axis of both.  A lane owns one (column, slice) cell, consecutive
// lanes take consecutive slices of a column, so the stores of a node pair's run are contiguous and
// the loads follow the plane table (consecutive planes apart from the wrap at HII_D_PARA).
// Both kernels are HBM-bound: 12 B per cell and field for the slabs (two loads, one store), 12 B
// (16 B with tau_21) per cell for dv/dr.
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

// the field pointers of one launch travel as a kernel argument (uniform index: scalar loads)
struct SlabFields {
    const float *lo[C21HIP_LC_MAX_FIELDS];
    const float *hi[C21HIP_LC_MAX_FIELDS];
    float *dst[C21HIP_LC_MAX_FIELDS];
};

// out = (w_lo a + w_hi b) / w_norm in fp64, stored as fp32 (lightconers.py:307-309); mean_max:
// where the fp32 product a*b < 0 the larger of the two (:311-313)
template <typename Index>
__global__ void __launch_bounds__(kBlock)
lightcone_slab_kernel(SlabFields f, int n_fields, unsigned mean_max, Index n_cols, Index run,
                      int d_para, long dst_stride, long dst_off,
                      const c21hip_lc_slice *__restrict__ tab, double w_norm) {
    const Index total = n_cols * run;
    for (Index t = (Index)blockIdx.x * kBlock + threadIdx.x; t < total;
         t += (Index)gridDim.x * kBlock) {
        const Index col = t / run;
        const Index j = t - col * run;
        const c21hip_lc_slice s = tab[j];
        const size_t src = (size_t)col * (size_t)d_para + (size_t)s.plane;
        const size_t dst = (size_t)col * (size_t)dst_stride + (size_t)dst_off + (size_t)j;
        for (int q = 0; q < n_fields; ++q) {
            const float a = f.lo[q][src];
            const float b = f.hi[q][src];
            float v = (float)((s.w_lo * (double)a + s.w_hi * (double)b) / w_norm);
            if (((mean_max >> q) & 1u) && a * b < 0.0f) v = a > b ? a : b;
            f.dst[q][dst] = v;
        }
    }
}

// np.gradient(v, dx, axis=-1, edge_order=2) on a non-periodic line of sight: central differences
// inside, second-order one-sided at both ends; then the Taylor form clipped at +-MAX_DVDR H
// (rsds.py:81-87) or, with a spin temperature, the fp64 tau_21 form (:88-101).
__global__ void __launch_bounds__(kBlock)
lightcone_dvdr_kernel(float *__restrict__ bt, const float *__restrict__ vel,
                      const float *__restrict__ tau, const double *__restrict__ hubble,
                      size_t n_cols, int n, double dx, double max_dvdr, int use_ts) {
    const size_t total = n_cols * (size_t)n;
    for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < total;
         t += (size_t)gridDim.x * kBlock) {
        const int k = (int)(t % (size_t)n);
        const float *v = vel + (t - (size_t)k); // the column
        double grad;
        if (k == 0) {
            grad = (-1.5 / dx) * (double)v[0] + (2. / dx) * (double)v[1] + (-0.5 / dx) * (double)v[2];
        } else if (k == n - 1) {
            grad = (0.5 / dx) * (double)v[n - 3] + (-2. / dx) * (double)v[n - 2] +
                   (1.5 / dx) * (double)v[n - 1];
        } else {
            grad = ((double)v[k + 1] - (double)v[k - 1]) / (2. * dx);
        }
        const double H = hubble[k];
        if (!use_ts) {
            const double mx = max_dvdr * H;
            const double d = grad < -mx ? -mx : (grad > mx ? mx : grad);
            bt[t] = (float)((double)bt[t] / fabs(1.0 + d / H));
        } else {
            const double ta = (double)tau[t];
            const double g = fabs(1.0 + grad / H);
            double fac = (1.0 - exp(-ta / g)) / (1.0 - exp(-ta));
            if (ta < 1e-10) fac = 1.0;
            bt[t] = bt[t] * (float)fac;
        }
    }
}
}  // namespace

extern "C" int c21hip_lightcone_slab(const float *const *lo, const float *const *hi, float *const *dst,
                                     int n_fields, unsigned mean_max, size_t n_cols, int run, int d_para,
                                     long dst_stride, long dst_off, const c21hip_lc_slice *tab,
                                     double w_norm, void *stream) {
    if (n_fields < 1 || n_fields > C21HIP_LC_MAX_FIELDS || run < 1 || d_para < 1 ||
        dst_off < 0 || dst_off + run > dst_stride) {
        c21hip_set_error("lightcone slab: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    SlabFields f{};
    for (int q = 0; q < n_fields; ++q) {
        f.lo[q] = lo[q];
        f.hi[q] = hi[q];
        f.dst[q] = dst[q];
    }
    const size_t total = n_cols * (size_t)run;
    if (total == 0) return 0;
    if (total <= 0xFFFFFFFFull - (size_t)kBlock * kMaxBlocks) { // 32-bit index: cheap column divide
        hipLaunchKernelGGL(lightcone_slab_kernel<uint32_t>, dim3(grid_for(total)), dim3(kBlock), 0,
                           (hipStream_t)stream, f, n_fields, mean_max, (uint32_t)n_cols, (uint32_t)run,
                           d_para, dst_stride, dst_off, tab, w_norm);
    } else {
        hipLaunchKernelGGL(lightcone_slab_kernel<size_t>, dim3(grid_for(total)), dim3(kBlock), 0,
                           (hipStream_t)stream, f, n_fields, mean_max, n_cols, (size_t)run, d_para,
                           dst_stride, dst_off, tab, w_norm);
    }
    LAUNCH_CHECK();
    return 0;
}

extern "C" int c21hip_lightcone_dvdr(float *bt, const float *vel, const float *tau, const double *hubble,
                                     size_t n_cols, int n_slices, double dx, double max_dvdr, int use_ts,
                                     void *stream) {
    if (n_slices < 3 || (use_ts && !tau)) {
        c21hip_set_error("lightcone dvdr: bad launch shape");
        return C21CM_VALUE_ERROR;
    }
    const size_t total = n_cols * (size_t)n_slices;
    if (total == 0) return 0;
    hipLaunchKernelGGL(lightcone_dvdr_kernel, dim3(grid_for(total)), dim3(kBlock), 0, (hipStream_t)stream,
                       bt, vel, tau, hubble, n_cols, n_slices, dx, max_dvdr, use_ts);
    LAUNCH_CHECK();
    return 0;
}

// rows of `width` bytes from a packed device slab into a host array of `dpitch`-byte rows
extern "C" int c21hip_d2h_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width,
                             size_t height, void *stream) {
    hipError_t e = hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost,
                                    (hipStream_t)stream);
    if (e != hipSuccess) {
        c21hip_set_error("hipMemcpy2DAsync: %s", hipGetErrorString(e));
        return C21CM_IO_ERROR;
    }
    return 0;
}
