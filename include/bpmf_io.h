/*
 * bpmf_io.h -- C ABI of the matrix file IO that the `bpmf` executable of this repo uses (also
 * exported from libbpmf_hip.so so that tests can check it against independent readers).
 *
 * Keeps the reference's file surface (c++/io.cpp:15-77,137-193): the format is chosen by the
 * extension, optionally followed by ".gz" (zlib):
 *   sparse: .mtx/.mm (MatrixMarket coordinate real|integer|pattern general), .sdm (binary:
 *           u64 nrow, ncol, nnz; u32 rows[nnz], cols[nnz] 1-based; f64 vals[nnz]), .sbm (same
 *           without values, read as 1.0)                          -- c++/io.cpp:256-314,414-522
 *   dense:  .ddm (u64 nrow, ncol; f64 column-major), .mtx/.mm (MatrixMarket array real general,
 *           column-major), .csv (nrow\n ncol\n rows of comma separated values) -- c++/io.cpp:195-254,318-409
 * Sparse matrices are returned as CSC with ascending rows per column and duplicate entries summed
 * (Eigen setFromTriplets, c++/io.cpp:282,521); explicit zeros are kept.
 * All functions return 0 or a negative code; bpmf_io_last_error() has the message
 * ("File '<name>' not found", c++/io.cpp:117).
 */
#ifndef BPMF_IO_H
#define BPMF_IO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#define BPMF_IO_API __attribute__((visibility("default")))
#else
#define BPMF_IO_API
#endif

BPMF_IO_API const char *bpmf_io_last_error(void);
/* arrays are malloc'ed by the library: release each with bpmf_io_free */
BPMF_IO_API int bpmf_io_read_sparse(const char *path, int64_t *nrows, int64_t *ncols, int64_t *nnz,
                                    int64_t **colptr, int32_t **rowidx, double **vals);
BPMF_IO_API int bpmf_io_write_sparse(const char *path, int64_t nrows, int64_t ncols, const int64_t *colptr,
                                     const int32_t *rowidx, const double *vals);
/* column-major */
BPMF_IO_API int bpmf_io_read_dense(const char *path, int64_t *nrows, int64_t *ncols, double **data);
BPMF_IO_API int bpmf_io_write_dense(const char *path, int64_t nrows, int64_t ncols, const double *data);
BPMF_IO_API void bpmf_io_free(void *p);
/* Sparse tensors of order 3 in the FROSTT .tns format (optionally .tns.gz): one entry per line, "i j t value", 1-based indices,
 * whitespace-separated, lines starting with # are comments.  _read_tns returns the entries in file order with 0-based indices and
 * dims[3] = the largest index seen per mode; it refuses a line with fewer or more than three indices, an index < 1, a value that is
 * not finite and a cell listed twice (the message names the line(s); the cell in 1-based indices).  _write_tns writes the values as
 * %.17g, so that a round trip is exact. */
BPMF_IO_API int bpmf_io_read_tns(const char *path, int64_t *nnz, int64_t *dims, int32_t **idx0, int32_t **idx1, int32_t **idx2, double **vals);
BPMF_IO_API int bpmf_io_write_tns(const char *path, int64_t nnz, const int32_t *idx0, const int32_t *idx1, const int32_t *idx2, const double *vals);

/* Saved models, format version 1: a directory DIR that a training run writes (bpmf --save-model DIR, gibbs(save_model=DIR)) and a
 * serving run loads (bpmf --model DIR, bpmf_amd.load_model).  Everything in the numbering of the input files.
 *   model.txt        `key value` lines, numbers as %.17g: bpmf_model 1, num_latent, rows, cols, samples, mean_rating, alpha,
 *                    likelihood gaussian|probit, probit_threshold, dtype f64|f32, hyper 0|1
 *   U-samples.ddm    (samples x num_latent) x rows, V-samples.ddm the same x cols: column c holds sample 0's num_latent values, then
 *                    sample 1's, ...: the layout of bpmf_hip_side_samples_get / _set
 *   U-hyper.ddm      with hyper 1, and V-hyper.ddm: (1 + num_latent + num_latent^2) x samples, column s = alpha_s, mu_s, Lambda_s as
 *                    bpmf_hip_side_hyper_get gives them
 * _write_model: Uh = Vh = NULL writes hyper 0.  _read_model: ints[7] = num_latent, rows, cols, samples, probit, f32, hyper;
 * reals[3] = mean_rating, alpha, probit_threshold; the four arrays are malloc'ed (Uh, Vh NULL with hyper 0).  It refuses, in one
 * line that names the file and the reason: an unknown version, a missing file or key, a row count that is not samples x
 * num_latent, sample counts that differ between the files, a value that is not finite. */
BPMF_IO_API int bpmf_io_write_model(const char *dir, int num_latent, int64_t rows, int64_t cols, int samples, double mean_rating, double alpha,
                                    int probit, double probit_threshold, int f32, const double *U, const double *V, const double *Uh,
                                    const double *Vh);
BPMF_IO_API int bpmf_io_read_model(const char *dir, int64_t *ints, double *reals, double **U, double **V, double **Uh, double **Vh);

/* Assignment of the columns of a side to `nparts` ranks (host; bpmf_amd/csrc/assign.cpp).
 * _greedy: Sys::assign of the reference (c++/assign.cpp:52-201, default weights): least-loaded rank on work = 10 + nnz,
 *   three sweeps, then a renumbering that makes every rank's columns contiguous -- order[new] = old column, dom[p] .. dom[p+1]
 *   = the new range of rank p.
 * _contiguous: cuts of the ORIGINAL order at equal c0 + nnz (no permutation: samples independent of the rank count). */
BPMF_IO_API int bpmf_assign_greedy(int64_t n, const int64_t *colptr, int nparts, int64_t *order, int64_t *dom);
BPMF_IO_API int bpmf_assign_contiguous(int64_t n, const int64_t *colptr, int nparts, double c0, int64_t *dom);

#ifdef __cplusplus
}
#endif
#endif
