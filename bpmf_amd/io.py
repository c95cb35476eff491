"""Matrix file IO through the library's C ABI (include/bpmf_io.h): the same readers / writers
the `bpmf` executable uses.  Formats by extension (.mtx .mm .sdm .sbm .ddm .csv, optional .gz);
sparse tensors of order 3 as FROSTT .tns (optional .gz)."""
import ctypes as C

import numpy as np

from . import _lib


class BpmfIoError(IOError):
    pass


def _check(lib, rc):
    if rc:
        raise BpmfIoError(lib.bpmf_io_last_error().decode("utf-8", "replace"))


def read_sparse(path):
    """Returns (nrows, ncols, (colptr int64, rowidx int32, vals f64)): CSC, rows sorted, duplicates summed."""
    lib = _lib.load_library()
    nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
    cp, ri, va = _lib.c_i64p(), _lib.c_i32p(), _lib.c_f64p()
    _check(lib, lib.bpmf_io_read_sparse(str(path).encode(), C.byref(nr), C.byref(nc), C.byref(nnz), C.byref(cp), C.byref(ri), C.byref(va)))
    try:
        colptr = np.ctypeslib.as_array(cp, shape=(nc.value + 1,)).copy()
        rowidx = np.ctypeslib.as_array(ri, shape=(max(nnz.value, 1),))[:nnz.value].copy()
        vals = np.ctypeslib.as_array(va, shape=(max(nnz.value, 1),))[:nnz.value].copy()
    finally:
        for p in (cp, ri, va):
            lib.bpmf_io_free(p)
    return nr.value, nc.value, (colptr, rowidx, vals)


def write_sparse(path, nrows, ncols, csc):
    lib = _lib.load_library()
    colptr = np.ascontiguousarray(csc[0], np.int64); rowidx = np.ascontiguousarray(csc[1], np.int32); vals = np.ascontiguousarray(csc[2], np.float64)
    _check(lib, lib.bpmf_io_write_sparse(str(path).encode(), int(nrows), int(ncols), colptr.ctypes.data, rowidx.ctypes.data, vals.ctypes.data))


def read_dense(path):
    """Returns an [nrows, ncols] array (the file is column-major)."""
    lib = _lib.load_library()
    nr, nc = C.c_int64(), C.c_int64()
    d = _lib.c_f64p()
    _check(lib, lib.bpmf_io_read_dense(str(path).encode(), C.byref(nr), C.byref(nc), C.byref(d)))
    try:
        n = nr.value * nc.value
        a = np.ctypeslib.as_array(d, shape=(max(n, 1),))[:n].copy()
    finally:
        lib.bpmf_io_free(d)
    return a.reshape((nc.value, nr.value)).T.copy()


def write_dense(path, a):
    lib = _lib.load_library()
    a = np.asarray(a, np.float64)
    cm = np.ascontiguousarray(a.T)                   # column-major bytes
    _check(lib, lib.bpmf_io_write_dense(str(path).encode(), a.shape[0], a.shape[1], cm.ctypes.data))


def read_tns(path):
    """A sparse tensor of order 3 from a FROSTT .tns file (optionally .tns.gz): one entry per line, `i j t value`, 1-based indices,
    whitespace-separated, `#` comment lines.  Returns (idx [nnz, 3] int32, 0-based, in file order; vals [nnz] float64; dims: the
    largest index seen per mode).  Refused with BpmfIoError naming the line: fewer or more than three indices, an index < 1, a value
    that is not finite, a cell listed twice (named in 1-based indices)."""
    lib = _lib.load_library()
    nnz = C.c_int64()
    dims = np.zeros(3, np.int64)
    ix = [_lib.c_i32p(), _lib.c_i32p(), _lib.c_i32p()]
    va = _lib.c_f64p()
    _check(lib, lib.bpmf_io_read_tns(str(path).encode(), C.byref(nnz), dims.ctypes.data, C.byref(ix[0]), C.byref(ix[1]), C.byref(ix[2]), C.byref(va)))
    try:
        n = nnz.value
        idx = np.stack([np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].copy() for p in ix], axis=1) if n else np.zeros((0, 3), np.int32)
        vals = np.ctypeslib.as_array(va, shape=(max(n, 1),))[:n].copy()
    finally:
        for p in ix + [va]:
            lib.bpmf_io_free(p)
    return idx, vals, tuple(int(d) for d in dims)


def write_tns(path, idx, vals):
    """Writes the entries (idx [nnz, 3], 0-based; vals [nnz]) as a FROSTT .tns file (.tns.gz: compressed), values as %.17g."""
    lib = _lib.load_library()
    idx = np.asarray(idx)
    vals = np.ascontiguousarray(vals, np.float64)
    if idx.ndim != 2 or idx.shape[1] != 3 or vals.shape != (idx.shape[0],):
        raise ValueError("write_tns: idx must be [nnz, 3] and vals [nnz]")
    cols = [np.ascontiguousarray(idx[:, m], np.int32) if len(vals) else np.zeros(1, np.int32) for m in range(3)]
    v = vals if len(vals) else np.zeros(1)
    _check(lib, lib.bpmf_io_write_tns(str(path).encode(), len(vals), cols[0].ctypes.data, cols[1].ctypes.data, cols[2].ctypes.data, v.ctypes.data))
