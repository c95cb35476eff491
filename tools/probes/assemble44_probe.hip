// Test aid (tests/test_gpu_assemble44.py): assemble44<K> of kernels.h on its own.  One wave loads the NB block accumulators
// and NG rhs sums of every lane from a file ((NB + NG) x 64 doubles, register-major), calls assemble44<K>, and the LDS images
// it leaves -- sA (K x LD, row-major) followed by sb (K) -- are written to a second file as raw doubles.
//   assemble44_probe K in.bin out.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.h"

using namespace bpmf;

template <int K>
__global__ __launch_bounds__(64) void k_probe(const double *__restrict__ in, double *__restrict__ out)
{
    using G = Geo44<K>;
    constexpr int LD = Geo1<K>::FLD, WORDS = K * LD + K;
    __shared__ __attribute__((aligned(16))) double lds[WORDS];
    const int lane = threadIdx.x;
    for (int t = lane; t < WORDS; t += 64) lds[t] = 0.0;
    __syncthreads();
    double acc[G::NB], rr[G::NG];
#pragma unroll
    for (int t = 0; t < G::NB; ++t) acc[t] = in[t * 64 + lane];
#pragma unroll
    for (int t = 0; t < G::NG; ++t) rr[t] = in[(G::NB + t) * 64 + lane];
    assemble44<K>(acc, rr, lds, lds + K * LD, LD, lane);
    __syncthreads();
    for (int t = lane; t < WORDS; t += 64) out[t] = lds[t];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

template <int K>
static int run(const char *fin, const char *fout)
{
    using G = Geo44<K>;
    constexpr int NIN = (G::NB + G::NG) * 64, NOUT = K * Geo1<K>::FLD + K;
    std::vector<double> h(NIN), o(NOUT);
    FILE *f = fopen(fin, "rb");
    if (!f || fread(h.data(), sizeof(double), NIN, f) != (size_t)NIN) { fprintf(stderr, "cannot read %d doubles from %s\n", NIN, fin); return 2; }
    fclose(f);
    double *din, *dout;
    CHECK(hipMalloc(&din, NIN * sizeof(double)));
    CHECK(hipMalloc(&dout, NOUT * sizeof(double)));
    CHECK(hipMemcpy(din, h.data(), NIN * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe<K>, dim3(1), dim3(64), 0, 0, din, dout);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(o.data(), dout, NOUT * sizeof(double), hipMemcpyDeviceToHost));
    f = fopen(fout, "wb");
    if (!f || fwrite(o.data(), sizeof(double), NOUT, f) != (size_t)NOUT) { fprintf(stderr, "cannot write %s\n", fout); return 2; }
    fclose(f);
    printf("assemble44<%d>: %d doubles in, %d out (LD %d)\n", K, NIN, NOUT, Geo1<K>::FLD);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s K in.bin out.bin\n", argv[0]); return 2; }
    switch (atoi(argv[1])) {
    case 8: return run<8>(argv[2], argv[3]);
    case 16: return run<16>(argv[2], argv[3]);
    case 32: return run<32>(argv[2], argv[3]);
    }
    fprintf(stderr, "K must be 8, 16 or 32\n");
    return 2;
}
