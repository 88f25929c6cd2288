"""The index as its rank blocks alone, for the tests: what `SVDSS search` makes resident when it has few reads to search
(svdss_index_load_blocks / svdss_index_attach_blocks on the "SVDSSBK1" section `SVDSS index` leaves behind the records of
its sidecar).  No text, no suffix array: k-mers with 1 to 4 occurrences are MULTI table entries, a unique interval is
walked by one rank step per symbol, the table order comes from SVDSS_LF_KMER.  tests/test_rank_blocks_host.py (CPU) and
tests/test_sfs_rank_only_gpu.py make their handles here, and tests/fuzz_gpu.py a third of its own."""
import ctypes as C
import os
import tempfile

import svdss_amd
from svdss_amd._lib import lib

EINVAL, EIO, ENODEV = 1, 3, 5      # include/svdss_hip.h

_ROUTE = [False]      # alternates: FMDIndex.load_blocks(file) / FMDIndex.load(file) followed by attach_blocks(file)


def expected_order(contigs, requested=None):
    """The order of the k-mer table a rank-only handle of these contigs gets (build_table, csrc/index_api.hip):
    min(requested, 14, max k with 4^k <= n), n = 2 * (bases + contigs); requested: SVDSS_LF_KMER, 13 when it is unset."""
    if requested is None:
        requested = int(os.environ.get("SVDSS_LF_KMER", "13"))
    n = 2 * (sum(len(c) for c in contigs) + len(contigs))
    k = max(0, min(requested, 14))
    while k > 0 and 4 ** k > n:
        k -= 1
    return k


def write_sidecar(full, path):
    """records + rank blocks of a full handle: the sidecar `SVDSS index` writes"""
    full.save_records(path)
    full.append_blocks(path)
    return path


def open_rank_only(path, route=None):
    """route True: load_blocks; False: load + attach_blocks; None: the two in turn from call to call"""
    if route is None:
        _ROUTE[0] = not _ROUTE[0]
        route = _ROUTE[0]
    if route:
        return svdss_amd.FMDIndex.load_blocks(path)
    return svdss_amd.FMDIndex.load(path).attach_blocks(path)


def rank_only(contigs, device=None, route=None, full=None, path=None):
    """(handle that holds the rank blocks alone -- not resident yet --, the table order it must get once it is).
    The index is built on the host (device=None) or in the HBM of `device`, written as records + blocks and read back."""
    if full is None:
        full = svdss_amd.FMDIndex.build(contigs, threads=2) if device is None else svdss_amd.FMDIndex.build(contigs, device=device)
    if path is not None:
        return open_rank_only(write_sidecar(full, path), route), expected_order(contigs)
    with tempfile.TemporaryDirectory() as tmp:
        return open_rank_only(write_sidecar(full, os.path.join(tmp, "ix.svdss")), route), expected_order(contigs)


def records_code(ix):
    """what svdss_index_records answers on this handle (a rank-only one holds none: SVDSS_ENODEV)"""
    rec, lens, n = C.c_void_p(), C.c_void_p(), C.c_int32(0)
    return lib.svdss_index_records(ix._h, C.byref(rec), C.byref(lens), C.byref(n))
