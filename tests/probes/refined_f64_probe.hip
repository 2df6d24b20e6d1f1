// refined_f64_probe.hip -- test-only: the two refined fp64 routines of the solver's pair
// arithmetic, rsqrt_sqrt_f64 and rcp_f64 (csrc/bb_solver_kernels.h), called once per operand so
// that tests/test_gpu_pair_math.py can hold each to the 2 ulp its comment claims.  Built by
// build.sh into tests/probes/librefined_f64_probe.so; never linked into the library.
#include "bb_solver_kernels.h"

namespace {
__global__ __launch_bounds__(256) void refined_f64_kernel(const double *__restrict__ x, int64_t n,
                                                          double *__restrict__ rinv,
                                                          double *__restrict__ dist,
                                                          double *__restrict__ rcp) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    rsqrt_sqrt_f64(x[i], rinv[i], dist[i]);
    rcp[i] = rcp_f64(x[i]);
}
}  // namespace

// x[n] on the host -> 1/sqrt(x), sqrt(x), 1/x as the routines give them.  0, or the HIP error.
extern "C" __attribute__((visibility("default"))) int bb_probe_refined_f64(const double *x, int64_t n,
                                                                           double *rinv, double *dist,
                                                                           double *rcp) {
    if (n <= 0) return 0;
    double *d = nullptr;
    const size_t bytes = (size_t)n * sizeof(double);
    hipError_t e = hipMalloc(&d, 4 * bytes);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, x, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        refined_f64_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(d, n, d + n, d + 2 * n, d + 3 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(rinv, d + n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dist, d + 2 * n, bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rcp, d + 3 * n, bytes, hipMemcpyDeviceToHost);
    hipFree(d);
    return (int)e;
}
