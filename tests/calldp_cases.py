"""Scoring parameters and sequence pairs shared by the tests of the call-side DP (tests/test_oracle_call.py pins the
oracle on them, tests/test_call_dp_shapes_gpu.py and tests/fuzz_gpu.py run the kernels on them)."""
import numpy as np

# (q, e, q2, e2), all with q + e <= q2 + e2: the order of the two gap pieces decides ties in the CIGAR, and ksw2's
# convention for the other order cannot be verified against the library here
GAP_MODELS = [(16, 2, 41, 1), (4, 2, 24, 1), (5, 3, 5, 3), (0, 1, 10, 1), (6, 1, 6, 2), (2, 4, 13, 2), (10, 1, 11, 1)]
MATRIX_KINDS = ("match", "random")
# the kernel's own edges: stripes of 64 target rows, blocks of 64 query columns, several wavefronts from 8 stripes on
STRIPE_EDGE_TL = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 576, 577, 1023, 1024, 1025]
BLOCK_EDGE_QL = [1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193]


def matrix(kind, m, rng):
    """m x m int8 substitution matrix, row = target symbol.  "match": a on the diagonal, -b elsewhere, and for m > 4 a
    last symbol that scores 0 against everything (ksw_gen_simple_mat with sc_ambi = 0, caller.cpp:336-337); "random":
    every entry drawn from -12..5, not symmetric; "extreme": random with the int8 limits -128 and 127 among the entries."""
    if kind == "match":
        a, b = int(rng.integers(1, 4)), int(rng.integers(1, 12))
        mat = np.full((m, m), -b, dtype=np.int8)
        np.fill_diagonal(mat, a)
        if m > 4:
            mat[m - 1, :] = 0
            mat[:, m - 1] = 0
    else:
        mat = rng.integers(-12, 6, size=(m, m)).astype(np.int8)
        if kind == "extreme":
            for v in (-128, 127, -128, 127):
                mat[int(rng.integers(0, m)), int(rng.integers(0, m))] = v
            mat[0, 1], mat[m - 1, 0] = -128, 127           # both limits are there whatever was overwritten
    return np.ascontiguousarray(mat.reshape(-1))


def resized(rng, t, ql, m=4, sub=0.01):
    """t made ql long by one indel at a random place, then about `sub` of the bases substituted"""
    tl = len(t)
    if ql > tl:
        at = int(rng.integers(0, tl + 1))
        q = np.concatenate([t[:at], rng.integers(0, m, size=ql - tl).astype(np.uint8), t[at:]])
    elif ql < tl:
        at = int(rng.integers(0, ql + 1))
        q = np.concatenate([t[:at], t[at + tl - ql:]])
    else:
        q = t.copy()
    hit = rng.random(ql) < sub
    q[hit] = rng.integers(0, m, size=int(hit.sum())).astype(np.uint8)
    return np.ascontiguousarray(q, dtype=np.uint8)


def small_pair(rng, m, indel):
    """a target of fewer than 60 symbols over 0..m-1 and a query: the target with substitutions and, if `indel`, one
    indel of up to 30; an unrelated query for the shortest targets"""
    tl = int(rng.integers(1, 60))
    t = rng.integers(0, m, size=tl).astype(np.uint8)
    if tl < 8 and not indel:
        return rng.integers(0, m, size=int(rng.integers(1, 50))).astype(np.uint8), t
    ql = max(1, tl + int(rng.integers(-30, 31))) if indel else tl
    return resized(rng, t, ql, m=m, sub=0.05), t
