// kernels_tensor.h -- sparse tensor factorisation (bpmf_hip_tensor_*, capi_tensor.hip; one translation unit: ktensor.hip).
// DESIGN.md section 22 has the model.
//
//   k_khatri_rao        P[:, e] = A[:, ia[e]] o B[:, ib[e]] for every entry e of a mode: the rows of the Khatri-Rao product of the two
//                       OTHER modes' factor matrices that the mode's entries select.  P (ld x n, column-major, ld = the context's leading
//                       dimension) is then "the other side" of the mode's unchanged column sampler: entry e of the mode rates row e.
//
// One fp64 multiply per element and nothing to contract it with: the result is the IEEE product bit for bit.  Rows
// kt .. ld - 1 (a padded num_latent) are WRITTEN as zeros, whatever the factor matrices hold there: P is shared by the three modes and
// by the test entries, so a launch may not count on what an earlier one left.
//
// k_khatri_rao: a lane owns two consecutive latent indices of one entry (one 16-byte load per operand, one 16-byte store), LD / 2 lanes
// own an entry, a wave 128 / LD entries.  The first lane of an entry loads its two indices, the others take them from it (one
// ds_bpermute each instead of LD / 2 loads of the same word).  No LDS, no atomics; entries past n issue nothing.  A plain one-thread-per-element
// form measured 1.29 - 1.43 x slower at every K and is not kept.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bpmf {

constexpr int kKhatriRaoBlock = 256;

template <int LD>
__global__ __launch_bounds__(kKhatriRaoBlock) void k_khatri_rao(const double *__restrict__ A, const double *__restrict__ B,
                                                                const int32_t *__restrict__ ia, const int32_t *__restrict__ ib, int64_t n,
                                                                int kt, double *__restrict__ P)
{
    static_assert(LD >= 8 && LD <= 128 && (LD & (LD - 1)) == 0, "LD: 8, 16, 32, 64 or 128");
    constexpr int LPE = LD / 2;                                       // lanes per entry
    constexpr int EPB = kKhatriRaoBlock / LPE;                        // entries per workgroup
    const int q = (int)threadIdx.x % LPE;                             // this lane's pair of latent indices: 2 q, 2 q + 1
    const int64_t e = (int64_t)blockIdx.x * EPB + (int)threadIdx.x / LPE;
    const bool live = e < n;
    int32_t ra = 0, rb = 0;
    if (live && q == 0) { ra = ia[e]; rb = ib[e]; }
    const int lane = (int)threadIdx.x & 63;                           // (an entry never straddles two waves: LPE divides 64)
    ra = __shfl(ra, lane - q);
    rb = __shfl(rb, lane - q);
    if (!live) return;
    const double2 a = *reinterpret_cast<const double2 *>(A + (int64_t)ra * LD + 2 * q);
    const double2 b = *reinterpret_cast<const double2 *>(B + (int64_t)rb * LD + 2 * q);
    double2 p;
    p.x = (2 * q < kt) ? a.x * b.x : 0.0;
    p.y = (2 * q + 1 < kt) ? a.y * b.y : 0.0;
    *reinterpret_cast<double2 *>(P + e * LD + 2 * q) = p;
}

}  // namespace bpmf
