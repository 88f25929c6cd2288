"""String collections for the BWT inversion tests (csrc/bwt_invert.h / bwt_invert.hip, svdss_bwt_strings): the shapes at
which marked LF walks can go wrong, a few thousand symbols each, in two BWT forms -- ropebwt's sentinel order
(tests/rld0_py.collection_bwt: the strings must come back exactly, in order) and this library's own
(FMDIndex.build(...).bwt(): the records and their reverse complements, as a multiset).  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import svdss_amd
from svdss_amd import synth
from svdss_amd._lib import lib
from tests import rld0_py

STRIDES = (1, 2, 3, 5, 7, 8, 64, 4096, 1 << 20)   # the last one is above every n here: sentinel walkers only
GUARD = 0xA5


def _rand(rng, n, alphabet=(1, 2, 3, 4)):
    return rng.choice(np.array(alphabet, np.uint8), size=n).astype(np.uint8)


def _to_rows(strings, want_mod):
    """the collection with its last string trimmed so that n = symbols + sentinels is want_mod modulo 128"""
    n = sum(len(s) for s in strings) + len(strings)
    cut = (n - want_mod) % 128
    assert len(strings[-1]) > cut
    out = list(strings[:-1]) + [strings[-1][:len(strings[-1]) - cut]]
    assert (sum(len(s) for s in out) + len(out)) % 128 == want_mod
    return out


@functools.lru_cache(maxsize=None)
def collections():
    """name -> list of nt6 uint8 arrays"""
    rng = np.random.default_rng(4711)
    pal = _rand(rng, 150)
    pal = np.concatenate([pal, synth.revcomp(pal)])            # equal to its own reverse complement
    with_n = _rand(rng, 900)
    with_n[100:140] = 5
    with_n[400:401] = 5
    with_n[640:900:7] = 5
    twin = _rand(rng, 333)
    c = {
        "lengths": [_rand(rng, l) for l in (0, 1, 2, 127, 128, 129, 300)],
        "rows_0_mod_128": _to_rows([_rand(rng, l) for l in (500, 77, 900)], 0),
        "rows_127_mod_128": _to_rows([_rand(rng, l) for l in (500, 77, 900)], 127),
        "all_a": [np.full(2000, 1, np.uint8), _rand(rng, 50)],
        "runs_of_n": [with_n, np.full(260, 5, np.uint8), _rand(rng, 40, (1, 2, 3, 4, 5))],
        "identical": [twin, _rand(rng, 90), twin.copy()],
        "own_revcomp": [pal, _rand(rng, 200)],
        "many_short": [_rand(rng, int(l)) for l in rng.integers(0, 41, size=700)],
        "one_record": [_rand(rng, 1500)],
    }
    assert np.array_equal(pal, synth.revcomp(pal))
    return c


@functools.lru_cache(maxsize=None)
def rope_bwt(name):
    """the collection's BWT with the sentinels in ropebwt's order: (bwt, the strings it must give back, in order)"""
    strings = collections()[name]
    return rld0_py.collection_bwt(strings), strings


@functools.lru_cache(maxsize=None)
def own_bwt(name):
    """the BWT of this library's index of the collection's non-empty records: (bwt, the sorted byte strings it stands for)"""
    recs = [s for s in collections()[name] if len(s)]
    ix = svdss_amd.FMDIndex.build(recs, threads=2)
    bwt = ix.bwt()
    ix.close()
    want = sorted([bytes(r) for r in recs] + [bytes(synth.revcomp(r)) for r in recs])
    return bwt, want


def raw_strings(bwt, device, stride, shift=0):
    """svdss_bwt_strings itself, the output buffer between guard bytes and `shift` bytes off its alignment:
    (status, list of byte strings or None, number of strings reported).  Asserts that the guards come back untouched."""
    b = np.ascontiguousarray(bwt, np.uint8)
    n = int(b.size)
    m = int((b == 0).sum())
    front = 64 + shift
    buf = np.full(front + (n - m) + 64, GUARD, np.uint8)
    lens = np.full(m + 2, -7, np.int64)
    k = C.c_int32(-1)
    rc = lib.svdss_bwt_strings(b.ctypes.data, n, device, stride, buf.ctypes.data + front, n - m, lens.ctypes.data + 8, m, C.byref(k))
    assert (buf[:front] == GUARD).all() and (buf[front + n - m:] == GUARD).all(), "guard bytes around the output were written"
    assert lens[0] == -7 and lens[-1] == -7, "guard words around the lengths were written"
    if rc != 0:
        return rc, None, k.value
    at = np.concatenate([[0], np.cumsum(lens[1:1 + m])])
    assert at[-1] == n - m
    body = buf[front:front + n - m]
    return rc, [bytes(body[at[r]:at[r + 1]]) for r in range(m)], k.value


def numpy_walk(bwt):
    """the strings by the plain LF walk, one per sentinel row (the reference the library's walks are held against)"""
    b = np.asarray(bwt, np.int64)
    n = len(b)
    acc = np.concatenate([[0], np.cumsum(np.bincount(b, minlength=6))])
    occ = np.zeros(n, np.int64)                      # occ[i] = number of b[i] in b[:i]
    for c in range(6):
        at = np.flatnonzero(b == c)
        occ[at] = np.arange(len(at))
    lf = acc[b] + occ
    out = []
    for r in range(int(acc[1])):
        s, i = [], r
        while b[i] != 0:
            s.append(int(b[i]))
            i = int(lf[i])
        out.append(bytes(s[::-1]))
    return out
