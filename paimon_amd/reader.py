"""Python mirror of the reader surface over the C-ABI (ctypes).

This is plumbing for tests/bench — the host side of the product is the C++
in libpaimon_hip.so (the reference's host side is compiled (Java) code, so
ours is C++ behind a C ABI; INTEGRATION.md shows the JNI binding a Java
deployment would use instead of this module).

Mirrors SplitRead<KeyValue>.createReader (operation/SplitRead.java:39-63) /
RecordReader (paimon-common/.../reader/RecordReader.java:40-72): a
MergeReadPlan yields one batch per section; batches reuse buffers
(releaseBatch contract) — copy out if you keep them.

The product path FAILS LOUDLY when the HIP library or a GPU is missing:
there is no CPU fallback here (the CPU restatement lives in oracle/ and is
test infrastructure only).
"""

import ctypes
import json
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpaimon_hip.so")

_DT_NP = {1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64,
          5: np.float32, 6: np.float64,
          7: np.int32,  # PMH_DT_STRING: global-dictionary ids
          8: np.bool_}  # PMH_DT_BOOL: one 0/1 byte per row

# enum pmh_logical: the annotation of an INT32/INT64 column. Values are
# handed out as the plain integers (days, milliseconds of the day,
# milliseconds / microseconds since the epoch); nothing converts to datetime
# on the read path.
(LT_NONE, LT_DATE, LT_TIME_MILLIS, LT_TIMESTAMP_MILLIS, LT_TIMESTAMP_MICROS,
 LT_TIMESTAMP_LTZ_MILLIS, LT_TIMESTAMP_LTZ_MICROS) = range(7)


class _Col(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("dtype", ctypes.c_int32),
                ("data", ctypes.c_void_p), ("valid", ctypes.c_void_p),
                ("dict_data", ctypes.c_void_p),
                ("dict_offsets", ctypes.POINTER(ctypes.c_int32)),
                ("dict_len", ctypes.c_int32),
                ("precision", ctypes.c_int32), ("scale", ctypes.c_int32),
                ("logical", ctypes.c_int32)]


class _Batch(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int32),
                ("device", ctypes.c_int32), ("cols", ctypes.POINTER(_Col))]


class _Stats(ctypes.Structure):
    _fields_ = [("rows_in", ctypes.c_int64), ("rows_out", ctypes.c_int64),
                ("hbm_bytes_algo", ctypes.c_int64),
                ("decode_ms", ctypes.c_double),
                ("partition_ms", ctypes.c_double),
                ("merge_ms", ctypes.c_double), ("scan_ms", ctypes.c_double),
                ("emit_ms", ctypes.c_double),
                ("total_device_ms", ctypes.c_double),
                ("h2d_ms", ctypes.c_double),
                ("path_mode", ctypes.c_int64),
                ("gpu_zstd_pages", ctypes.c_int64),
                ("lookup_ms", ctypes.c_double)]


_lib = None


def load_lib(required=True):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if required:
            raise RuntimeError(
                f"libpaimon_hip.so missing at {LIB_PATH} — build it with "
                "`make -C paimon_amd/csrc` (no CPU fallback exists; the HIP "
                "path is the product).")
        return None
    lib = ctypes.CDLL(LIB_PATH)
    lib.pmh_open_session.restype = ctypes.c_void_p
    lib.pmh_open_session.argtypes = [ctypes.c_int]
    lib.pmh_close_session.argtypes = [ctypes.c_void_p]
    lib.pmh_plan_create.restype = ctypes.c_void_p
    lib.pmh_plan_create.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.pmh_read_next.restype = ctypes.c_int64
    lib.pmh_read_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Batch)]
    lib.pmh_changelog_next.restype = ctypes.c_int64
    lib.pmh_changelog_next.argtypes = [ctypes.c_void_p,
                                       ctypes.POINTER(_Batch)]
    lib.pmh_plan_close.argtypes = [ctypes.c_void_p]
    lib.pmh_plan_reset.argtypes = [ctypes.c_void_p]
    lib.pmh_plan_reset.restype = ctypes.c_int
    lib.pmh_stats_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Stats)]
    lib.pmh_last_error.restype = ctypes.c_char_p
    lib.pmh_debug_footer_json.restype = ctypes.c_void_p
    lib.pmh_debug_footer_json.argtypes = [ctypes.c_char_p]
    lib.pmh_free_string.argtypes = [ctypes.c_void_p]
    lib.pmh_write_parquet.restype = ctypes.c_int
    lib.pmh_write_parquet.argtypes = [
        ctypes.POINTER(_Col), ctypes.c_int32, ctypes.c_int64,
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_char_p]
    lib.pmh_debug_parse_dv.restype = ctypes.c_int64
    lib.pmh_debug_parse_dv.argtypes = [
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64,
        ctypes.POINTER(ctypes.c_int64), ctypes.c_int64]
    lib.pmh_debug_interval_partition.restype = ctypes.c_int
    lib.pmh_debug_interval_partition.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_int32)]
    lib.pmh_debug_lookup_probe.restype = ctypes.c_int
    lib.pmh_debug_lookup_probe.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
        ctypes.c_int64, ctypes.POINTER(ctypes.c_int32),
        ctypes.POINTER(ctypes.c_int64)]
    lib.pmh_debug_json_i64.restype = ctypes.c_int
    lib.pmh_debug_json_i64.argtypes = [ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_int64)]
    _lib = lib
    return lib


def last_error():
    return load_lib().pmh_last_error().decode()


def debug_footer(path):
    lib = load_lib()
    p = lib.pmh_debug_footer_json(path.encode())
    if not p:
        raise RuntimeError(last_error())
    s = ctypes.string_at(p).decode()
    lib.pmh_free_string(p)
    return json.loads(s)


_NP_DT = {np.dtype(np.int8): 1, np.dtype(np.int16): 2,
          np.dtype(np.int32): 3, np.dtype(np.int64): 4,
          np.dtype(np.float32): 5, np.dtype(np.float64): 6,
          np.dtype(np.bool_): 8}


def write_parquet(path, columns, row_group_rows=0, page_rows=0,
                  compression="NONE", dicts=None, decimals=None,
                  logicals=None):
    """Write a Parquet v1 data file via the native writer
    (pmh_write_parquet) — the compaction write-back path. `columns` is an
    ordered list of (name, values[, valid]) with numpy arrays; valid
    None/omitted = REQUIRED column.

    dicts: {name: sequence of bytes/str} — the column's values are int32
    ids into that dictionary; written as a BYTE_ARRAY column with a
    dictionary page + RLE_DICTIONARY data pages (the reference writer's
    default for strings).
    decimals: {name: (precision, scale)} — int32/int64 unscaled values
    written with the DECIMAL annotation (INT32 p<=9 / INT64 p<=18,
    ParquetSchemaConverter.java:153-171).
    logicals: {name: LT_*} — int32 (date, time) / int64 (timestamp) values
    written with that annotation. numpy bool columns are written as BOOLEAN,
    bit-packed."""
    lib = load_lib()
    dicts = dicts or {}
    decimals = decimals or {}
    logicals = logicals or {}
    n_rows = len(columns[0][1]) if columns else 0
    arrs = []  # keep contiguous buffers alive
    cols = (_Col * len(columns))()
    for i, col in enumerate(columns):
        name, vals = col[0], np.ascontiguousarray(col[1])
        valid = col[2] if len(col) > 2 else None
        if vals.dtype not in _NP_DT:
            raise ValueError(f"unsupported dtype {vals.dtype} for {name}")
        if len(vals) != n_rows:
            raise ValueError("ragged columns")
        arrs.append(vals)
        cols[i].name = name.encode()
        cols[i].dtype = _NP_DT[vals.dtype]
        cols[i].data = vals.ctypes.data_as(ctypes.c_void_p)
        if name in dicts:
            if vals.dtype != np.int32:
                raise ValueError(f"{name}: dictionary ids must be int32")
            entries = [e.encode() if isinstance(e, str) else bytes(e)
                       for e in dicts[name]]
            blob = b"".join(entries)
            offs = np.zeros(len(entries) + 1, dtype=np.int32)
            np.cumsum([len(e) for e in entries], out=offs[1:])
            blob_arr = np.frombuffer(blob, dtype=np.uint8).copy() if blob \
                else np.zeros(1, dtype=np.uint8)
            arrs += [blob_arr, offs]
            cols[i].dtype = 7
            cols[i].dict_data = blob_arr.ctypes.data_as(ctypes.c_void_p)
            cols[i].dict_offsets = offs.ctypes.data_as(
                ctypes.POINTER(ctypes.c_int32))
            cols[i].dict_len = len(entries)
        elif name in decimals:
            p, s = decimals[name]
            cols[i].precision = int(p)
            cols[i].scale = int(s)
        elif logicals.get(name):
            cols[i].logical = int(logicals[name])
        if valid is not None:
            v8 = np.ascontiguousarray(np.asarray(valid, dtype=np.uint8))
            if len(v8) != n_rows:
                raise ValueError("ragged validity")
            arrs.append(v8)
            cols[i].valid = v8.ctypes.data_as(ctypes.c_void_p)
        else:
            cols[i].valid = None
    rc = lib.pmh_write_parquet(cols, len(columns), n_rows, path.encode(),
                               row_group_rows, page_rows,
                               compression.encode())
    if rc != 0:
        raise RuntimeError(f"pmh_write_parquet: {last_error()}")


def debug_parse_dv(path, offset=0, length=0, cap=1 << 22):
    lib = load_lib()
    out = np.empty(cap, dtype=np.int64)
    n = lib.pmh_debug_parse_dv(
        path.encode(), offset, length,
        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cap)
    if n < 0:
        raise RuntimeError(last_error())
    return out[:min(n, cap)].copy()


def debug_zstd_cpu(data, cap=None):
    """Decode one zstd frame with the scalar zstd_core.h restatement on the
    host (test entry; the GPU page decoder shares the same core)."""
    lib = load_lib()
    lib.pmh_debug_zstd_cpu.restype = ctypes.c_int64
    lib.pmh_debug_zstd_cpu.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_int64]
    data = bytes(data)
    if cap is None:
        cap = max(16, len(data) * 64)
    out = np.empty(cap, dtype=np.uint8)
    n = lib.pmh_debug_zstd_cpu(data, len(data),
                               out.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 0:
        raise RuntimeError(last_error())
    return bytes(out[:n])


def debug_zstd_gpu(data, expected_size):
    """Decode one zstd frame on the GPU (k_zstd_pages); requires a device."""
    lib = load_lib()
    lib.pmh_debug_zstd_gpu.restype = ctypes.c_int64
    lib.pmh_debug_zstd_gpu.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_void_p, ctypes.c_int64]
    data = bytes(data)
    out = np.empty(max(1, expected_size), dtype=np.uint8)
    n = lib.pmh_debug_zstd_gpu(data, len(data),
                               out.ctypes.data_as(ctypes.c_void_p),
                               expected_size)
    if n < 0:
        raise RuntimeError(last_error())
    return bytes(out[:n])


def debug_zstd_enc_cpu(data, cap=None):
    """Compress one zstd frame with the scalar zstd_core.h encoder (host).
    Tests prove the frames decode with libzstd (pyarrow)."""
    lib = load_lib()
    lib.pmh_debug_zstd_enc_cpu.restype = ctypes.c_int64
    lib.pmh_debug_zstd_enc_cpu.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_int64]
    data = bytes(data)
    if cap is None:
        cap = len(data) + (len(data) >> 8) + 1024
    out = np.empty(cap, dtype=np.uint8)
    n = lib.pmh_debug_zstd_enc_cpu(data, len(data),
                                   out.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 0:
        raise RuntimeError(last_error())
    return bytes(out[:n])


def debug_zstd_enc_gpu(data, cap=None):
    """Compress one zstd frame ON THE GPU (k_zstd_compress batch of 1)."""
    lib = load_lib()
    lib.pmh_debug_zstd_enc_gpu.restype = ctypes.c_int64
    lib.pmh_debug_zstd_enc_gpu.argtypes = [ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_int64]
    data = bytes(data)
    if cap is None:
        cap = len(data) + (len(data) >> 8) + 1024
    out = np.empty(cap, dtype=np.uint8)
    n = lib.pmh_debug_zstd_enc_gpu(data, len(data),
                                   out.ctypes.data_as(ctypes.c_void_p), cap)
    if n < 0:
        raise RuntimeError(last_error())
    return bytes(out[:n])


ORC_INTS_SIGNED, ORC_INTS_UNSIGNED, ORC_INTS_BYTE = 0, 1, 2
ORC_INTS_HOST, ORC_INTS_PRESCAN, ORC_INTS_DEVICE = 0, 1, 2


def debug_orc_ints(stream, n_values, kind, mode, out_esize=8, src_shift=0):
    """One ORC integer stream through the product's decoders
    (pmh_debug_orc_ints). mode ORC_INTS_HOST returns the host LENGTH
    decoder's values as uint64 (n_values < 0: until the stream ends);
    ORC_INTS_PRESCAN returns the number of device chunks; ORC_INTS_DEVICE
    returns what k_rlev2 wrote, as int32/int64 by out_esize (needs a GPU).
    Raises RuntimeError on a rejected stream; a device store outside the
    output raises AssertionError."""
    lib = load_lib()
    lib.pmh_debug_orc_ints.restype = ctypes.c_int64
    lib.pmh_debug_orc_ints.argtypes = [
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int64]
    stream = bytes(stream)

    def call(out, cap):
        ptr = out.ctypes.data_as(ctypes.c_void_p) if out is not None else None
        n = lib.pmh_debug_orc_ints(stream, len(stream), n_values, kind,
                                   out_esize, mode, src_shift, ptr, cap)
        if n == -2:
            raise AssertionError(last_error())
        if n < 0:
            raise RuntimeError(last_error())
        return n

    if mode == ORC_INTS_PRESCAN:
        return call(None, 0)
    if mode == ORC_INTS_HOST:
        n = call(None, 0) if n_values < 0 else n_values
        out = np.empty(max(n, 1), dtype=np.uint64)
        n = call(out, len(out))
        return out[:n]
    out = np.empty(max(n_values, 1),
                   dtype=np.int32 if out_esize == 4 else np.int64)
    call(out, len(out))
    return out[:n_values]


ORC_DECIMAL_HOST, ORC_DECIMAL_DEVICE = 0, 2
ORC_DECIMAL_FULL_RANGE = 19  # precision: the whole int64 range


def debug_orc_decimal(data, n_values, precision, scale, mode, scales=None,
                      out_esize=8, src_shift=0):
    """One ORC DECIMAL DATA stream (zigzag varints) through the product's
    decoder (pmh_debug_orc_decimal). scales: per-value data scales, None =
    all at the column scale. ORC_DECIMAL_HOST runs the prescan and the
    scalar core on the host; ORC_DECIMAL_DEVICE returns what k_orc_varint
    wrote (needs a GPU). Returns unscaled values at the column scale as
    int32/int64 by out_esize. Raises RuntimeError on a rejected stream or
    value; a device store outside the output raises AssertionError."""
    lib = load_lib()
    lib.pmh_debug_orc_decimal.restype = ctypes.c_int64
    lib.pmh_debug_orc_decimal.argtypes = [
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    data = bytes(data)
    sc = None
    if scales is not None:
        sc = np.ascontiguousarray(scales, dtype=np.int32)
        if len(sc) != n_values:
            raise ValueError("scales must hold n_values entries")
    out = np.empty(max(n_values, 1),
                   dtype=np.int32 if out_esize == 4 else np.int64)
    n = lib.pmh_debug_orc_decimal(
        data, len(data),
        sc.ctypes.data_as(ctypes.c_void_p) if sc is not None else None,
        precision, scale, n_values, out_esize, mode, src_shift,
        out.ctypes.data_as(ctypes.c_void_p), len(out))
    if n == -2:
        raise AssertionError(last_error())
    if n < 0:
        raise RuntimeError(last_error())
    return out[:n_values]


BITS_LSB, BITS_MSB = 0, 1          # bit order inside a byte
BITS_RAW, BITS_BYTE_RLE = 0, 1     # Parquet PLAIN bits / ORC boolean RLE
BITS_HOST, BITS_DEVICE = 0, 2


def debug_bits(stream, n_values, bit_order, fmt, mode, out_esize=1,
               src_shift=0, out_shift=0):
    """One BOOLEAN value stream through the product's decoder
    (pmh_debug_bits): raw LSB/MSB-first bits (a Parquet PLAIN page payload)
    or an ORC boolean byte-RLE stream. BITS_HOST runs the prescan and the
    scalar core on the host; BITS_DEVICE returns what k_bits_expand wrote
    (needs a GPU), the output starting out_shift elements past an aligned
    address. Returns uint8 (out_esize 1) or int32 (out_esize 4) values,
    untouched elements still 0xA5.. in device mode. Raises RuntimeError on a
    rejected stream; a device store outside the output raises
    AssertionError."""
    lib = load_lib()
    lib.pmh_debug_bits.restype = ctypes.c_int64
    lib.pmh_debug_bits.argtypes = [
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
        ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    stream = bytes(stream)
    out = np.full(max(n_values, 1), 0xA5A5A5A5 if out_esize == 4 else 0xA5,
                  dtype=np.uint32 if out_esize == 4 else np.uint8)
    n = lib.pmh_debug_bits(stream, len(stream), n_values, bit_order, fmt,
                           out_esize, mode, src_shift, out_shift,
                           out.ctypes.data_as(ctypes.c_void_p), len(out))
    if n == -2:
        raise AssertionError(last_error())
    if n < 0:
        raise RuntimeError(last_error())
    out = out[:n_values]
    return out.view(np.int32) if out_esize == 4 else out


ORC_TS_MILLIS, ORC_TS_MICROS = 0, 1
ORC_TS_HOST, ORC_TS_DEVICE = 0, 2


def debug_orc_timestamp(data, secondary, n_values, unit, mode):
    """One ORC TIMESTAMP stream pair (DATA: signed RLEv2 seconds relative
    to 2015-01-01; SECONDARY: unsigned RLEv2 nanos with trailing zeros
    removed) through the product's decoders (pmh_debug_orc_timestamp).
    Returns int64 milliseconds or microseconds since the epoch by unit.
    ORC_TS_HOST needs no GPU; ORC_TS_DEVICE runs k_rlev2 + k_orc_timestamp.
    Raises RuntimeError on a rejected stream or a refused value; a device
    store outside the output raises AssertionError."""
    lib = load_lib()
    lib.pmh_debug_orc_timestamp.restype = ctypes.c_int64
    lib.pmh_debug_orc_timestamp.argtypes = [
        ctypes.c_char_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
        ctypes.c_int64]
    data, secondary = bytes(data), bytes(secondary)
    out = np.empty(max(n_values, 1), dtype=np.int64)
    n = lib.pmh_debug_orc_timestamp(
        data, len(data), secondary, len(secondary), n_values, unit, mode,
        out.ctypes.data_as(ctypes.c_void_p), len(out))
    if n == -2:
        raise AssertionError(last_error())
    if n < 0:
        raise RuntimeError(last_error())
    return out[:n_values]


def debug_check_column(path, column, type_str):
    """Check one column of a Parquet / ORC data file against a declared
    plan type the way staging does, without a plan or a GPU
    (pmh_debug_check_column). Raises RuntimeError with the text plan
    creation would fail with."""
    lib = load_lib()
    lib.pmh_debug_check_column.restype = ctypes.c_int
    lib.pmh_debug_check_column.argtypes = [ctypes.c_char_p, ctypes.c_char_p,
                                           ctypes.c_char_p]
    if lib.pmh_debug_check_column(path.encode(), column.encode(),
                                  type_str.encode()) != 0:
        raise RuntimeError(last_error())


def interval_partition(min_keys, max_keys):
    """Returns (section_id, run_id) per input file, per the IntervalPartition
    restatement in libpaimon_hip (plan.cpp)."""
    lib = load_lib()
    n = len(min_keys)
    mn = (ctypes.c_int64 * n)(*[int(x) for x in min_keys])
    mx = (ctypes.c_int64 * n)(*[int(x) for x in max_keys])
    sec = (ctypes.c_int32 * n)()
    run = (ctypes.c_int32 * n)()
    ns = lib.pmh_debug_interval_partition(n, mn, mx, sec, run)
    if ns < 0:
        raise RuntimeError(last_error())
    return list(sec), list(run), ns


def debug_json_i64(text):
    """Parse one JSON number string through the plan descriptor's parser
    (JsonParser + as_i64) and return the int64 it yields; raises on a
    malformed or out-of-range number."""
    lib = load_lib()
    out = ctypes.c_int64(0)
    if lib.pmh_debug_json_i64(str(text).encode(), ctypes.byref(out)) != 0:
        raise RuntimeError(last_error())
    return out.value


def debug_lookup_probe(levels, queries):
    """Point lookup of `queries` into `levels` (a list of ascending unique
    int64 key arrays, searched in list order; first hit wins) through the
    host entry of the search core that k_lookup_probe runs on the GPU.
    Returns (level, row) int arrays; -1 where no level holds the key."""
    lib = load_lib()
    lv = [np.ascontiguousarray(a, dtype=np.int64) for a in levels]
    q = np.ascontiguousarray(queries, dtype=np.int64)
    n = len(lv)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in lv])
    rows = (ctypes.c_int64 * max(n, 1))(*[len(a) for a in lv])
    out_level = np.empty(len(q), dtype=np.int32)
    out_row = np.empty(len(q), dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    rc = lib.pmh_debug_lookup_probe(
        n, ptrs, rows, q.ctypes.data_as(i64p), len(q),
        out_level.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
        out_row.ctypes.data_as(i64p))
    if rc != 0:
        raise RuntimeError(last_error())
    return out_level, out_row


PARTITION_HOST = 0
PARTITION_DEVICE = 1


def debug_partition(runs, tile_rows, mode=PARTITION_HOST):
    """Merge-path partition cuts of `runs` (a list of ascending unique key
    arrays, all int64 or all int32) through pmh_debug_partition: the shared
    search core on the host (PARTITION_HOST) or the partition kernels alone
    (PARTITION_DEVICE). Returns an int32 array [n_bounds, k]."""
    lib = load_lib()
    dt = np.dtype(runs[0].dtype)
    if dt not in (np.dtype(np.int64), np.dtype(np.int32)):
        raise ValueError("keys must be int64 or int32")
    ks = [np.ascontiguousarray(a, dtype=dt) for a in runs]
    k = len(ks)
    total = sum(len(a) for a in ks)
    n_bounds = (total + tile_rows - 1) // tile_rows + 1
    ptrs = (ctypes.c_void_p * k)(
        *[a.ctypes.data if len(a) else None for a in ks])
    lens = (ctypes.c_int64 * k)(*[len(a) for a in ks])
    cuts = np.empty((n_bounds, k), dtype=np.int32)
    lib.pmh_debug_partition.restype = ctypes.c_int
    lib.pmh_debug_partition.argtypes = [
        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int64,
        ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    rc = lib.pmh_debug_partition(
        k, ptrs, lens, dt.itemsize, tile_rows, mode,
        cuts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != 0:
        raise RuntimeError(last_error())
    return cuts


EMIT_NONE, EMIT_GATHER, EMIT_CONTIG, EMIT_STREAM = 0, 1, 2, 3


def debug_last_emit_kernel():
    """The kernel the last winner emit of this process ran: EMIT_GATHER
    (k_emit), EMIT_CONTIG (k_emit_contig), EMIT_STREAM (k_emit_stream), or
    EMIT_NONE before the first one."""
    lib = load_lib()
    lib.pmh_debug_last_emit_kernel.restype = ctypes.c_int
    lib.pmh_debug_last_emit_kernel.argtypes = []
    return int(lib.pmh_debug_last_emit_kernel())


PU_EMIT_NONE, PU_EMIT_OVERLAY, PU_EMIT_SG, PU_EMIT_SGA = 0, 1, 2, 3


def debug_last_pu_emit_kernel():
    """The partial-update emit kernel the last read of this process
    launched: PU_EMIT_OVERLAY (k_emit_pu), PU_EMIT_SG (k_emit_pu_sg),
    PU_EMIT_SGA (k_emit_pu_sga, aggregate functions inside sequence groups),
    or PU_EMIT_NONE before the first one."""
    lib = load_lib()
    lib.pmh_debug_last_pu_emit_kernel.restype = ctypes.c_int
    lib.pmh_debug_last_pu_emit_kernel.argtypes = []
    return int(lib.pmh_debug_last_pu_emit_kernel())


PU_AGG_CODES = {"last_non_null_value": 0, "last_value": 1, "first_value": 2,
                "first_non_null_value": 3, "sum": 4, "max": 5, "min": 6}
PU_AGG_IGNORE_RETRACT = 0x80
PU_AGG_NONE = 0xff


def debug_pu_agg_fold(kinds, dtypes, values, valid, col_group, sg_fields,
                      sg_nseq, col_agg, ignore_delete=False):
    """One key group through the partial-update aggregate fold on the host
    (pmh_debug_pu_agg_fold; the core k_emit_pu_sga runs). kinds [n] RowKind
    bytes in merge order; values / valid [n, n_cols] (values as int64 bits);
    dtypes, col_group, col_agg [n_cols]; sg_fields [n_groups, 4]; sg_nseq
    [n_groups]. Returns (values [n_cols] int64, valid [n_cols] bool, kind,
    last member index or -1, unsupported-retraction flag)."""
    lib = load_lib()
    kinds = np.ascontiguousarray(kinds, np.int8)
    dtypes = np.ascontiguousarray(dtypes, np.uint8)
    values = np.ascontiguousarray(values, np.int64)
    valid = np.ascontiguousarray(valid, np.uint8)
    col_group = np.ascontiguousarray(col_group, np.uint8)
    sg_fields = np.ascontiguousarray(sg_fields, np.int16).reshape(-1)
    sg_nseq = np.ascontiguousarray(sg_nseq, np.uint8)
    col_agg = np.ascontiguousarray(col_agg, np.uint8)
    n, n_cols = len(kinds), len(dtypes)
    assert values.shape == (n, n_cols) and valid.shape == (n, n_cols)
    assert len(col_group) == n_cols and len(col_agg) == n_cols
    assert len(sg_fields) == 4 * len(sg_nseq)
    out_v = np.zeros(n_cols, np.int64)
    out_ok = np.zeros(n_cols, np.uint8)
    kind = ctypes.c_int32(0)
    last = ctypes.c_int32(0)
    unsup = ctypes.c_int32(0)
    fn = lib.pmh_debug_pu_agg_fold
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                   ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.POINTER(ctypes.c_int32),
                   ctypes.POINTER(ctypes.c_int32),
                   ctypes.POINTER(ctypes.c_int32)]
    rc = fn(n, kinds.ctypes.data, n_cols, dtypes.ctypes.data,
            values.ctypes.data, valid.ctypes.data, len(sg_nseq),
            col_group.ctypes.data, sg_fields.ctypes.data or None,
            sg_nseq.ctypes.data or None, col_agg.ctypes.data,
            int(bool(ignore_delete)), out_v.ctypes.data, out_ok.ctypes.data,
            ctypes.byref(kind), ctypes.byref(last), ctypes.byref(unsup))
    if rc != 0:
        raise RuntimeError(last_error())
    return out_v, out_ok.astype(bool), kind.value, last.value, \
        bool(unsup.value)


class Session:
    def __init__(self, device=0):
        self.lib = load_lib()
        self.h = self.lib.pmh_open_session(device)
        if not self.h:
            raise RuntimeError(f"pmh_open_session: {last_error()}")
        self.device = device

    def close(self):
        if self.h:
            self.lib.pmh_close_session(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class MergeReadPlan:
    """One bucket's merge-on-read plan (MergeFileSplitRead.createReader)."""

    def __init__(self, session: Session, files, key_cols, value_cols,
                 merge_engine="deduplicate", drop_delete=True,
                 ignore_delete=False, output="host", aggregations=None,
                 remove_record_on_delete=False, sequence_groups=None,
                 ignore_retract=None, sequence_fields=None,
                 changelog_producer=None, changelog_row_dedup=False,
                 max_level=None, sort_engine="loser-tree", filters=None,
                 lookup_files=None, default_aggregation=None):
        self.lib = session.lib
        desc = {
            "key_cols": key_cols,
            "value_cols": value_cols,
            "merge_engine": merge_engine,
            "drop_delete": drop_delete,
            "ignore_delete": ignore_delete,
            "remove_record_on_delete": remove_record_on_delete,
            "output": output,
            "sort_engine": sort_engine,
            "files": files,
        }
        if sequence_groups:
            # fields.<seq>.sequence-group=<members> (CoreOptions):
            # [{"sequence_fields": [...], "group_fields": [...]}]
            desc["sequence_groups"] = list(sequence_groups)
        if ignore_retract:
            # fields.<f>.ignore-retract = true (FieldIgnoreRetractAgg)
            desc["ignore_retract"] = list(ignore_retract)
        if sequence_fields:
            # sequence.field (UserDefinedSeqComparator): value columns that
            # compare before the sequence number
            desc["sequence_fields"] = list(sequence_fields)
        if aggregations:
            # fields.<name>.aggregate-function (CoreOptions FIELDS_PREFIX);
            # aggregation: unnamed columns default to last_non_null_value;
            # partial-update: the named columns are fields of a sequence
            # group (last_non_null_value alone needs none)
            desc["aggregations"] = dict(aggregations)
        if default_aggregation:
            # fields.default-aggregate-function (partial-update): every
            # value column that is neither a sequence field nor named in
            # aggregations
            desc["default_aggregation"] = str(default_aggregation)
        if filters:
            # value-filter conjunction; pushed into SINGLE-RUN sections
            # only (MergeFileSplitRead.java:227-239) — overlapping
            # sections emit unfiltered, as the reference reader does
            desc["filters"] = list(filters)
        if changelog_producer:
            # changelog-producer = full-compaction
            # (FullChangelogMergeFunctionWrapper; max_level = num-levels - 1)
            # or lookup (LookupChangelogMergeFunctionWrapper; lookup_files =
            # the data files of the levels above the output level)
            desc["changelog_producer"] = changelog_producer
            desc["changelog_row_deduplicate"] = bool(changelog_row_dedup)
            desc["max_level"] = int(max_level if max_level is not None
                                    else -1)
        if lookup_files:
            desc["lookup_files"] = list(lookup_files)
        self.h = self.lib.pmh_plan_create(session.h,
                                          json.dumps(desc).encode())
        if not self.h:
            raise RuntimeError(f"pmh_plan_create: {last_error()}")
        self.output = output
        # name -> LT_* of the date / time / timestamp columns, as the batches
        # report it (compaction hands it to the writer)
        self.logicals = {}

    def read_next(self):
        """Returns dict name -> numpy array (host output mode), or a raw
        _Batch with device pointers (device mode); None at end of input."""
        b = _Batch()
        n = self.lib.pmh_read_next(self.h, ctypes.byref(b))
        if n < 0:
            raise RuntimeError(f"pmh_read_next: {last_error()}")
        if n == 0 and b.n_cols == 0:
            return None
        if self.output == "device":
            return b
        out = {}
        for c in range(b.n_cols):
            col = b.cols[c]
            dt = np.dtype(_DT_NP[col.dtype])
            name = col.name.decode()
            if b.n_rows and col.data:
                buf = ctypes.cast(
                    col.data,
                    ctypes.POINTER(ctypes.c_uint8 * (b.n_rows * dt.itemsize)))
                arr = np.frombuffer(bytes(buf.contents), dtype=dt)
            else:
                arr = np.empty(0, dtype=dt)
            out[name] = arr
            if col.logical:
                self.logicals[name] = int(col.logical)
            if col.dtype == 7 and col.dict_len > 0:
                # dictionary string column: values are global ids; expose
                # the dictionary as an object array of bytes
                offs = np.ctypeslib.as_array(col.dict_offsets,
                                             shape=(col.dict_len + 1,))
                blob = ctypes.cast(
                    col.dict_data,
                    ctypes.POINTER(ctypes.c_uint8 * int(offs[-1])))
                bb = bytes(blob.contents) if offs[-1] else b""
                out[name + "#dict"] = np.array(
                    [bb[offs[j]:offs[j + 1]] for j in range(col.dict_len)],
                    dtype=object)
            if col.valid and b.n_rows:
                vbuf = ctypes.cast(col.valid,
                                   ctypes.POINTER(ctypes.c_uint8 * b.n_rows))
                out[name + "#valid"] = np.frombuffer(
                    bytes(vbuf.contents), dtype=np.uint8).astype(bool)
        return out

    def read_changelog(self):
        """Changelog batch of the LAST read_next (changelog_producer =
        "full-compaction" or "lookup"): dict name -> numpy array (host
        output), may be empty. Same schema as the main batch; _VALUE_KIND
        carries the changelog RowKind (0=+I, 1=-U, 2=+U, 3=-D)."""
        b = _Batch()
        n = self.lib.pmh_changelog_next(self.h, ctypes.byref(b))
        if n < 0:
            raise RuntimeError(f"pmh_changelog_next: {last_error()}")
        if self.output == "device":
            return b
        out = {}
        for c in range(b.n_cols):
            col = b.cols[c]
            dt = np.dtype(_DT_NP[col.dtype])
            name = col.name.decode()
            if b.n_rows and col.data:
                buf = ctypes.cast(
                    col.data,
                    ctypes.POINTER(ctypes.c_uint8 * (b.n_rows * dt.itemsize)))
                arr = np.frombuffer(bytes(buf.contents), dtype=dt)
            else:
                arr = np.empty(0, dtype=dt)
            out[name] = arr
            if col.valid and b.n_rows:
                vbuf = ctypes.cast(col.valid,
                                   ctypes.POINTER(ctypes.c_uint8 * b.n_rows))
                out[name + "#valid"] = np.frombuffer(
                    bytes(vbuf.contents), dtype=np.uint8).astype(bool)
        return out

    def reset(self):
        """Rewind to the first section without restaging (bench repeats)."""
        if self.lib.pmh_plan_reset(self.h) != 0:
            raise RuntimeError(last_error())

    def stats(self):
        s = _Stats()
        if self.lib.pmh_stats_get(self.h, ctypes.byref(s)) != 0:
            raise RuntimeError(last_error())
        return {f: getattr(s, f) for f, _ in s._fields_}

    def close(self):
        if self.h:
            self.lib.pmh_plan_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def file_descs_from_metas(metas):
    out = []
    for m in metas:
        d = {"path": m["path"], "rowCount": m["rowCount"],
             "minKey": m["minKey"], "maxKey": m["maxKey"],
             "level": m.get("level", 0)}
        if m.get("deletionVector"):
            # DeletionFile {path, offset, length}
            d["deletionVector"] = m["deletionVector"]
        out.append(d)
    return out
