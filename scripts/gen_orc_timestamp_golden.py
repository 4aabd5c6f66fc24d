"""Generate the ORC TIMESTAMP fixtures under tests/golden/.

pyarrow's ORC writer (and its reader, for TIMESTAMP columns) resolves the
writer timezone through an IANA zoneinfo directory, which a test machine may
not have; so the files are committed, with what pyarrow itself reads back
from them stored beside each as .npy. This script points TZDIR at the
installed `tzdata` package's zoneinfo and needs nothing else.

Per run i (three runs x 2 000 rows, sorted unique int64 keys that overlap
between runs, globally unique sequence numbers, 10 % deletes):
  tests/golden/orc_ts_run{i}.orc   _KEY_k, _SEQUENCE_NUMBER, _VALUE_KIND,
                                   v_ts: nullable timestamp[us] (ORC
                                   TIMESTAMP), all values at or after 1970
  tests/golden/orc_ts_run{i}.npy   int64 [5, n]: key, seq, kind, pyarrow's
                                   read-back of v_ts in microseconds (0 where
                                   null), validity

Usage: python scripts/gen_orc_timestamp_golden.py
"""

import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
N_RUNS, ROWS = 3, 2000


def main():
    spec = importlib.util.find_spec("tzdata")
    if spec is None:
        sys.exit("the tzdata package is needed (its zoneinfo directory)")
    os.environ["TZDIR"] = os.path.join(os.path.dirname(spec.origin),
                                       "zoneinfo")
    import numpy as np
    import pyarrow as pa
    from pyarrow import orc as pa_orc

    rng = np.random.default_rng(20261020)
    space = N_RUNS * ROWS * 3 // 2
    seqs = rng.permutation(N_RUNS * ROWS).astype(np.int64)
    for i in range(N_RUNS):
        key = np.sort(rng.choice(space, ROWS, replace=False)).astype(np.int64)
        seq = seqs[i * ROWS:(i + 1) * ROWS]
        kind = np.where(rng.random(ROWS) < 0.1, 3, 0).astype(np.int8)
        # seconds from 1970 up to 2100, fractions with every count of
        # trailing zeros (the writer strips them into the 3-bit code)
        secs = rng.integers(0, 4_102_444_800, ROWS, dtype=np.int64)
        zeros = rng.integers(0, 7, ROWS)
        micros = (rng.integers(0, 10 ** 6, ROWS) // 10 ** zeros) * 10 ** zeros
        ts = secs * 10 ** 6 + micros
        ts[:6] = [0, 1, 999_999, 1_000_000, 1_420_070_400_000_000,
                  4_102_444_799_999_999]
        valid = rng.random(ROWS) >= 0.3
        valid[:6] = True
        tbl = pa.Table.from_arrays(
            [pa.array(key), pa.array(seq), pa.array(kind),
             pa.array(ts, pa.timestamp("us"), mask=~valid)],
            schema=pa.schema([
                pa.field("_KEY_k", pa.int64(), nullable=False),
                pa.field("_SEQUENCE_NUMBER", pa.int64(), nullable=False),
                pa.field("_VALUE_KIND", pa.int8(), nullable=False),
                pa.field("v_ts", pa.timestamp("us"))]))
        path = os.path.join(GOLDEN, f"orc_ts_run{i}.orc")
        pa_orc.write_table(tbl, path, compression="uncompressed")
        back = pa_orc.read_table(path)
        col = back.column("v_ts").combine_chunks()
        got_valid = np.asarray(col.is_valid())
        got = np.asarray(col.cast(pa.timestamp("us")).cast(pa.int64())
                         .fill_null(0))
        assert (got_valid == valid).all()
        assert (got[valid] == ts[valid]).all(), "pyarrow round trip"
        np.save(os.path.join(GOLDEN, f"orc_ts_run{i}.npy"),
                np.stack([key, seq, kind.astype(np.int64), got,
                          got_valid.astype(np.int64)]))
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
