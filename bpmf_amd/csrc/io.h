// io.h -- matrix files of the bpmf command line (see include/bpmf_io.h for the formats).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace bpmf {
namespace io {

struct IoError : std::runtime_error { using std::runtime_error::runtime_error; };

struct Csc {                       // sorted rows per column, duplicates summed
    int64_t nrows = 0, ncols = 0;
    std::vector<int64_t> colptr;   // ncols + 1
    std::vector<int32_t> rowidx;
    std::vector<double> vals;
    int64_t dup_row = -1, dup_col = -1;   // the first cell the file listed more than once (0-based; -1: none)
    int64_t nnz() const { return colptr.empty() ? 0 : colptr.back(); }
};

struct Dense {                     // column-major
    int64_t nrows = 0, ncols = 0;
    std::vector<double> data;
};

enum class Kind { none, sdm, sbm, mtx, csv, ddm };
struct FileType { Kind kind = Kind::none; bool gz = false; };
FileType file_type(const std::string &path);

// triplets (0-based) -> CSC; rows sorted, duplicates summed, explicit zeros kept
Csc csc_from_triplets(int64_t nrows, int64_t ncols, const std::vector<int32_t> &rows, const std::vector<int32_t> &cols,
                      const std::vector<double> &vals);
Csc transpose(const Csc &m);
// grows the shape without touching the entries (conservativeResize, c++/sample.cpp:119-122)
void resize(Csc &m, int64_t nrows, int64_t ncols);

// a Matrix Market file in coordinate (sparse) format; false for an array file, another kind or an unreadable file
bool mtx_is_coordinate(const std::string &path);
Csc read_sparse(const std::string &path);
Dense read_dense(const std::string &path);
void write_sparse(const std::string &path, const Csc &m);
void write_dense(const std::string &path, const Dense &m);

// a sparse tensor of order 3 in the FROSTT .tns format (optionally .gz): one entry per line, "i j t value", 1-based indices,
// whitespace-separated, # comment lines.  Entries in file order, indices 0-based here; dims: the largest index seen per mode.
struct Tns {
    int64_t dims[3] = {0, 0, 0};
    std::vector<int32_t> idx[3];
    std::vector<double> vals;
    std::vector<int64_t> line;     // the line of every entry (read_tns; for messages)
};
// refuses (IoError naming the line): fewer or more than three indices, an index < 1 or past 32 bits, a value that is not finite,
// a cell listed twice
Tns read_tns(const std::string &path);
void write_tns(const std::string &path, const Tns &t);      // values as %.17g: a round trip is exact

// a saved model, format version 1: a directory with model.txt (`key value` lines, numbers as %.17g),
// U-samples.ddm ((S K) x rows) and V-samples.ddm ((S K) x cols) -- column c holds sample 0's K values, then sample 1's ..., the
// layout of bpmf_hip_side_samples_get -- and, with hyper, U-hyper.ddm and V-hyper.ddm ((1 + K + K^2) x S: column s holds alpha_s,
// mu_s, Lambda_s as bpmf_hip_side_hyper_get gives them).  Everything in the numbering of the input files.
struct Model {
    int K = 0, S = 0;
    int64_t rows = 0, cols = 0;                  // users, movies
    double mean_rating = 0.0, alpha = 0.0, probit_threshold = 0.0;
    bool probit = false, f32 = false, hyper = false;
    std::vector<double> U, V, Uh, Vh;            // the four matrices, column-major (Uh, Vh empty without hyper)
};
void write_model(const std::string &dir, const Model &m);        // creates dir when it is missing
// refuses (IoError, one line naming the file and the reason): an unknown version, a missing file or key, a row count that is not
// S K (1 + K + K^2), a column count that is not rows / cols (S), a value that is not finite
Model read_model(const std::string &dir);

}  // namespace io
}  // namespace bpmf
