"""`fastx` in the rotation of tests/fuzz_gpu.py: the device parser of `search --fastx` (svdss_amd/csrc/fastx_device.hip)
on seeded small files against tests/mirror/fastx.py, the generators of tests/fastx_cases.py.

    python -m tests.fuzz_fastx --what fastx --minutes 2 --seed 1        (or any list of tests.fuzz_gpu's names)

tests/fuzz_gpu.py stays as it is; this module adds its entry to the table and runs the same main."""
import numpy as np

from tests import fastx_cases as FC, fuzz_gpu
from tests.fuzz_gpu import Mismatch
from tests.mirror import fastx as M


def fuzz_fastx(rng, out_dir, it):
    from svdss_amd import fastxdev
    data, batch, pieces = FC.fuzz_file(rng)
    chunks = FC.chunks_of(data, batch, pieces)
    want, want_declined, want_rest = M.plan(chunks, batch)
    blob = M.bgzf_pack(pieces) if pieces is not None else data
    names, flat, offs, declined_at, st = fastxdev.parse_fastx(blob, batch, bgzf=pieces is not None)
    ok = (names == [n for n, _ in want] and flat.tobytes() == b"".join(M.nt6(s) for _, s in want) and
          list(np.diff(offs)) == [len(s) for _, s in want] and declined_at == want_declined and st["rest"] == want_rest)
    if not ok:
        path = f"{out_dir}/fastx_{it}.bin"
        with open(path, "wb") as fh:
            fh.write(data)
        raise Mismatch(f"device parser and mirror differ (batch {batch}, {'BGZF' if pieces is not None else 'plain'}, "
                       f"declined {declined_at} / {want_declined}): {path}")
    return len(want), f"{len(want)} records, {len(chunks)} batches, declined at {declined_at}"


fuzz_gpu.FUZZERS["fastx"] = fuzz_fastx

if __name__ == "__main__":
    fuzz_gpu.main()
