"""The search kernel on the index as its rank blocks alone -- the form `SVDSS search`, `smooth --index --sfs` and `run`
make resident when there are few reads to search (svdss_index_load_blocks / svdss_index_attach_blocks) -- against the
oracle: table entries without a suffix array (MULTI of size 1..4), lanes without TEXT / SET / BS modes, the table order
of SVDSS_LF_KMER, the launch plan of this form, replicas that keep no host copy, and the <uint64_t> instantiation without
a suffix array (SVDSS_FORCE_SA64 on the blocks' loader).  Every handle comes from tests/rank_only_cases.py and every test
asserts the table order that form must have, so none can run the full form unnoticed.  Integer work: bit-exact."""
import ctypes as C

import numpy as np
import pytest

import svdss_amd
from svdss_amd import synth
from svdss_amd._lib import SvdssError, check, lib
from tests import oracle_lib as O
from tests import rank_only_cases as R
from tests.common import from_ascii, load_golden, small_workload

pytestmark = pytest.mark.gpu

KNOBS = ("SVDSS_LF_KMER", "SVDSS_FORCE_SA64", "SVDSS_SEGMENTS", "SVDSS_KMER", "SVDSS_FALLBACK_DIRECT", "SVDSS_ORDER", "SVDSS_BS",
         "SVDSS_SET", "SVDSS_TABLE_FORWARD", "SVDSS_TICKETS", "SVDSS_BLOCKS", "SVDSS_EXTRA_LDS", "SVDSS_LF_ONLY", "SVDSS_INDEX_NO_CACHE")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(params=[False, True], ids=["narrow", "wide"])
def wide(request, monkeypatch):
    """SVDSS_FORCE_SA64 unset / set: 32- and 64-bit intervals (sfs_search2_kernel<uint32_t / uint64_t>)"""
    if request.param:
        monkeypatch.setenv("SVDSS_FORCE_SA64", "1")
    return request.param


def _resident(contigs, **kw):
    """a rank-only handle of these contigs, resident on GPU 0, with the table order this form must have"""
    ix, k = R.rank_only(contigs, device=0, **kw)
    ix.to_device(0)
    assert ix.kmer_k == k, (ix.kmer_k, k)
    assert R.records_code(ix) == R.ENODEV
    return ix, k


def _search(ix, flat, offs, assemble):
    pp = svdss_amd.PingPong(ix, assemble=assemble)
    got = pp.ping_pong_search(flat, offs)
    info = {"segments": pp.last_segments, "fallbacks": pp.last_fallbacks, "bs": pp.last_used_bs}
    pp.close()
    return got, info


def _same(got, want, what=None):
    c, q, l, e = want
    assert (got.counts == c).all() and (got.n_ext == e).all(), what
    assert len(got.qs) == len(q) and (got.qs == q).all() and (got.len == l).all(), what


def _against_oracle(ix, fm, reads, what=None):
    flat, offs = svdss_amd.pack_reads(reads)
    out = None
    for assemble in (False, True):
        want = fm.search_batch(flat, offs, assemble)
        got, info = _search(ix, flat, offs, assemble)
        _same(got, want, (what, assemble))
        out = want if out is None else out
    return out


# ---- shared references and oracle results: computed once, never changed

_CACHE = {}


def _golden(tmp_path_factory):
    """the golden cases as sidecars (records + blocks), written once"""
    if "golden" not in _CACHE:
        d = tmp_path_factory.mktemp("golden_rank_only")
        out = []
        for case in load_golden():
            contigs = [from_ascii(c) for c in case["contigs"]]
            path = R.write_sidecar(svdss_amd.FMDIndex.build(contigs, device=0), str(d / (case["name"] + ".svdss")))
            flat, offs = svdss_amd.pack_reads([from_ascii(r["read"]) for r in case["reads"]])
            out.append((case, contigs, path, flat, offs))
        _CACHE["golden"] = out
    return _CACHE["golden"]


def _case_b(seed, tmp_path_factory):
    """test_sfs_gpu.py::test_random_reads_match_oracle's workload, its oracle results and its sidecar"""
    key = ("b", seed)
    if key not in _CACHE:
        ref, hap, svs, flat, offs = small_workload(seed=seed, n_reads=300, read_len=2000)
        fm = O.OracleFMD.build(ref)
        want = {a: fm.search_batch(flat, offs, a) for a in (False, True)}
        assert want[False][0].sum() > 0
        path = R.write_sidecar(svdss_amd.FMDIndex.build(ref, device=0), str(tmp_path_factory.mktemp(f"b{seed}") / "ix.svdss"))
        _CACHE[key] = (ref, flat, offs, want, path)
    return _CACHE[key]


def _open_resident(path, contigs):
    ix = R.open_rank_only(path).to_device(0)
    assert ix.kmer_k == R.expected_order(contigs), (ix.kmer_k, R.expected_order(contigs))
    return ix


# ---- a. golden vectors

@pytest.mark.parametrize("segments", ["1", "4"])
@pytest.mark.parametrize("lf_kmer", [None, "0", "1", "5"])
def test_golden_vectors(lf_kmer, segments, wide, monkeypatch, tmp_path_factory):
    """The committed brute-force vectors: SFS, assembled SFS and extension counts without a table, with tables of order 1
    and 5 and with the default order, which every one of these small references clamps (4^K <= n)."""
    if lf_kmer is not None:
        monkeypatch.setenv("SVDSS_LF_KMER", lf_kmer)
    monkeypatch.setenv("SVDSS_SEGMENTS", segments)
    for case, contigs, path, flat, offs in _golden(tmp_path_factory):
        ix = _open_resident(path, contigs)
        if lf_kmer is None:
            n = 2 * (sum(len(c) for c in contigs) + len(contigs))
            assert ix.kmer_k < 13 and 4 ** ix.kmer_k <= n < 4 ** (ix.kmer_k + 1), case["name"]      # the clamp
        else:
            assert ix.kmer_k == int(lf_kmer)
        raw, _ = _search(ix, flat, offs, False)
        for got, rd, ne in zip(raw.per_read(), case["reads"], raw.n_ext.tolist()):
            assert [list(x) for x in got] == rd["sfs"], case["name"]
            assert ne == rd["n_ext"], case["name"]
        asm, _ = _search(ix, flat, offs, True)
        for got, rd in zip(asm.per_read(), case["reads"]):
            assert [list(x) for x in got] == rd["assembled"], case["name"]
        ix.close()


# ---- b. random reads

@pytest.mark.parametrize("seed", [31, 32])
def test_random_reads_match_oracle(seed, wide, monkeypatch, tmp_path_factory):
    """n = 460,004 symbols: the default order clamps to 9.  Several lanes per read by default, one under
    SVDSS_SEGMENTS=1: the same SFS either way."""
    ref, flat, offs, want, path = _case_b(seed, tmp_path_factory)
    ix = _open_resident(path, ref)
    assert ix.kmer_k == 9 and ix.size == 460004
    for assemble in (False, True):
        got, info = _search(ix, flat, offs, assemble)
        assert info["segments"] > 1 and not info["bs"]
        _same(got, want[assemble])
        monkeypatch.setenv("SVDSS_SEGMENTS", "1")
        got1, info1 = _search(ix, flat, offs, assemble)
        monkeypatch.delenv("SVDSS_SEGMENTS")
        assert info1["segments"] == 1
        _same(got1, want[assemble])


def test_order_is_capped_by_the_text_not_by_the_request(monkeypatch):
    """530,000 bases: n = 1,060,002 >= 4^10; SVDSS_LF_KMER=14 still gives 10."""
    monkeypatch.setenv("SVDSS_LF_KMER", "14")
    ref, hap, svs, flat, offs = small_workload(seed=34, ref_lens=(530000,), n_reads=200, read_len=2000)
    ix, k = _resident(ref)
    assert k == 10 and ix.kmer_k == 10
    fm = O.OracleFMD.build(ref)
    for assemble in (False, True):
        got, _ = _search(ix, flat, offs, assemble)
        _same(got, fm.search_batch(flat, offs, assemble))


# ---- c. edges

def test_empty_ragged_and_unaligned():
    ref, hap, svs, flat, offs = small_workload(seed=41, n_reads=10, read_len=300, ref_lens=(40000,))
    reads = [flat[offs[i]:offs[i + 1]] for i in range(10)]
    reads.insert(3, np.zeros(0, np.uint8))
    reads.append(np.zeros(0, np.uint8))
    reads.insert(0, ref[0][5:6])
    ix, k = _resident(ref)
    assert k == 8
    c = _against_oracle(ix, O.OracleFMD.build(ref), reads)[0]
    assert c[4] == 0 and c[-1] == 0
    got, _ = _search(ix, np.zeros(0, np.uint8), np.zeros(1, np.int64), True)      # the empty batch
    assert len(got.counts) == 0 and len(got.qs) == 0


@pytest.mark.parametrize("lf_kmer", ["0", "7"])
def test_batches_smaller_than_one_fetch(lf_kmer, monkeypatch):
    """A whole batch of fewer than 64 symbols is searched in a padded copy: one read of 1 .. 63 symbols, several tiny
    reads, only empty reads; without a table and with the largest one this reference allows."""
    monkeypatch.setenv("SVDSS_LF_KMER", lf_kmer)
    ref, hap, svs, flat, offs = small_workload(seed=43, n_reads=2, read_len=300, ref_lens=(20000,))
    fm = O.OracleFMD.build(ref)
    cases = [[ref[0][100:100 + n].copy()] for n in (1, 2, 15, 16, 17, 31, 47, 63)]
    cases += [[ref[0][7:20].copy(), np.zeros(0, np.uint8), hap[0][50:61].copy(), ref[0][900:925].copy()], [np.zeros(0, np.uint8)] * 3]
    ix, k = _resident(ref)
    assert k == int(lf_kmer)
    for reads in cases:
        _against_oracle(ix, fm, reads, [len(r) for r in reads])


def test_record_region_overflow_is_rerun_exactly():
    """an all-N read against an N-free reference: one SFS per base, far more than the default record region"""
    ref = synth.make_reference([30000], seed=7)
    ix, k = _resident(ref)
    assert k == 7
    reads = [np.full(500, 5, np.uint8), ref[0][100:900].copy(), np.full(64, 5, np.uint8), synth.revcomp(ref[0][2000:2600])]
    reads[1][400] = 5
    c = _against_oracle(ix, O.OracleFMD.build(ref), reads)[0]
    assert c[0] == 500


def test_reads_shorter_than_the_table_order_and_cut_by_n(tmp_path_factory):
    ref, flat, offs, want, path = _case_b(31, tmp_path_factory)
    ix = _open_resident(path, ref)
    assert ix.kmer_k == 9
    reads = [np.full(40, 5, np.uint8)] + [flat[offs[3]:offs[3] + n].copy() for n in (1, 2, 8, 9, 10, 16)]
    reads += [np.concatenate([flat[offs[7]:offs[7] + 500], np.full(3, 5, np.uint8), flat[offs[7] + 500:offs[7] + 900]]),
              np.concatenate([flat[offs[9]:offs[9] + 4], np.full(3, 5, np.uint8), flat[offs[9] + 4:offs[9] + 12]])]
    _against_oracle(ix, O.OracleFMD.build(ref), reads)


@pytest.mark.parametrize("lf_kmer", [None, "4", "14"])
def test_degenerate_references_and_reads(lf_kmer, monkeypatch):
    """test_sfs_gpu.py's degenerate records (1, 2, 15, 16, 17 bases, N only, one base repeated, another's reverse
    complement) and reads (1 .. K+1 bases, N only, a record, a record plus a base on either side), by both launch shapes."""
    if lf_kmer:
        monkeypatch.setenv("SVDSS_LF_KMER", lf_kmer)
    rng = np.random.default_rng(77)
    base = synth.make_reference([40000, 9000], seed=78, n_runs=(300,))
    tiny = [np.array(x, np.uint8) for x in ([1], [3, 2], [4] * 15, [2, 1, 4, 3] * 4, [1, 2, 3, 4, 1, 1, 2, 2, 3, 3, 4, 4, 2, 4, 1, 3, 2])]
    ref = base + tiny + [np.full(700, 5, np.uint8), np.full(3000, 2, np.uint8), synth.revcomp(base[1][1000:6000])]
    ix, k = _resident(ref)
    assert k == (4 if lf_kmer == "4" else 8)           # n = 115,522: 4^8 <= n < 4^9
    fm = O.OracleFMD.build(ref)
    reads = [np.array([c], np.uint8) for c in (1, 2, 3, 4, 5)]
    reads += [rng.integers(1, 5, size=n).astype(np.uint8) for n in (2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 127, 129)]
    reads += [np.full(n, 5, np.uint8) for n in (1, 16, 200)]
    reads += [t.copy() for t in tiny] + [synth.revcomp(t) for t in tiny]
    reads += [np.concatenate([[3], tiny[3]]), np.concatenate([tiny[3], [1]]), np.concatenate([[4], tiny[4], [4]])]
    reads += [base[0][100:3100].copy(), synth.revcomp(base[0][20000:23000]), base[1][990:6010].copy()]
    reads += [np.full(500, 2, np.uint8), np.full(3001, 2, np.uint8), np.full(40, 3, np.uint8)]
    hap, _ = synth.implant_svs(base, 3, seed=79, min_len=50, max_len=200)
    f2, o2, _ = synth.simulate_reads(hap, 40, 2500, 0.01, seed=80)
    reads += [f2[o2[i]:o2[i + 1]] for i in range(40)]
    flat, offs = svdss_amd.pack_reads(reads)
    for assemble in (False, True):
        want = fm.search_batch(flat, offs, assemble)
        for seg in (None, "1"):
            if seg:
                monkeypatch.setenv("SVDSS_SEGMENTS", seg)
            got, info = _search(ix, flat, offs, assemble)
            if seg:
                monkeypatch.delenv("SVDSS_SEGMENTS")
                assert info["segments"] == 1
            _same(got, want, (assemble, seg))
    c = want[0]
    hit = [i for i, r in enumerate(reads) if any(len(r) == len(t) and ((r == t).all() or (r == synth.revcomp(t)).all()) for t in tiny)]
    assert len(hit) >= 10 and all(c[i] == 0 for i in hit)


# ---- d. low-copy repeats with N runs

def test_low_copy_repeats_with_n_runs(wide):
    """Where the full index leaves for SET / TEXT mode (1..4 occurrences followed in the text), this form walks the
    intervals of 1..4 rows to the end of the phase by rank steps: the reference of
    test_lane_logic.py::test_v2_set_mode_in_low_copy_repeats, reads of both strands, every third with an N."""
    ref = synth.make_reference([400000], seed=3, repeat_frac=0.3, divergence=0.006, n_runs=(60,))
    rng = np.random.default_rng(5)
    reads = []
    for i in range(40):
        ln = int(rng.integers(1500, 5001))
        a = int(rng.integers(0, len(ref[0]) - ln))
        r = ref[0][a:a + ln].copy()
        e = rng.random(ln) < 0.005
        r[e] = (r[e] - 1 + rng.integers(1, 4, size=int(e.sum()))) % 4 + 1
        if i % 3 == 0:
            r[int(rng.integers(0, ln))] = 5
        reads.append(synth.revcomp(r.astype(np.uint8)) if i % 2 else r.astype(np.uint8))
    ix, k = _resident(ref)
    assert k == 9
    c = _against_oracle(ix, O.OracleFMD.build(ref), reads)[0]
    assert c.sum() > 40


# ---- e. segmented launches and the fallback ladder

@pytest.mark.parametrize("segments", ["1", "2", "4", "16"])
def test_segmented_search_is_exact(segments, monkeypatch):
    monkeypatch.setenv("SVDSS_SEGMENTS", segments)
    ref, hap, svs, flat, offs = small_workload(seed=38, n_reads=60, read_len=4000, ref_lens=(400000,), err=0.005)
    flat2, offs2, _ = synth.simulate_reads(hap, 60, 4000, 0.005, seed=39)              # (4,000 bases each, not ragged)
    reads = [flat2[offs2[i]:offs2[i + 1]] for i in range(60)]
    reads += [np.full(1500, 5, np.uint8), ref[0][:5000].copy(), np.zeros(0, np.uint8), ref[0][7:300].copy()]
    assert len(reads) == 64
    flat, offs = svdss_amd.pack_reads(reads)
    ix, k = _resident(ref)
    assert k == 9
    fm = O.OracleFMD.build(ref)
    for assemble in (False, True):
        got, info = _search(ix, flat, offs, assemble)
        assert info["segments"] == int(segments)
        if segments != "1":
            assert info["fallbacks"] > 0           # the all-N read cannot be stitched within the overrun
        _same(got, fm.search_batch(flat, offs, assemble))


_LADDER = {}


@pytest.mark.parametrize("n_reads,direct", [(24, None), (150, None), (150, "0"), (24, "1000000")])
def test_reads_with_long_novel_insertions_in_segmented_launches(n_reads, direct, monkeypatch):
    """What this form gets from `SVDSS smooth`: reads that equal the reference but for one long insertion of novel
    sequence.  The segment that owns it overflows its record region and the read goes down the fallback ladder --
    straight to one lane (few reads, or SVDSS_FALLBACK_DIRECT large) or through a level with a quarter of the segments
    (150 reads with SVDSS_FALLBACK_DIRECT=0)."""
    monkeypatch.setenv("SVDSS_SEGMENTS", "8")
    if direct is not None:
        monkeypatch.setenv("SVDSS_FALLBACK_DIRECT", direct)
    if "ref" not in _LADDER:
        _LADDER["ref"] = synth.make_reference([500000], seed=5)
        _LADDER["fm"] = O.OracleFMD.build(_LADDER["ref"])
    ref, fm = _LADDER["ref"], _LADDER["fm"]
    rng = np.random.default_rng(77)
    reads = []
    for k in range(n_reads):
        a = int(rng.integers(0, 500000 - 9000))
        r = ref[0][a:a + 8000].copy()
        ins = rng.integers(1, 5, size=int(rng.integers(300, 2001))).astype(np.uint8)
        cut = int(rng.integers(500, 7500))
        r = np.concatenate([r[:cut], ins, r[cut:]]) if k % 5 else r            # (every fifth read: a plain copy)
        if k % 7 == 3:
            r = synth.revcomp(r)
        reads.append(r)
    flat, offs = svdss_amd.pack_reads(reads)
    ix, k = _resident(ref)
    assert k == 9
    for assemble in (False, True):
        want = fm.search_batch(flat, offs, assemble)
        got, info = _search(ix, flat, offs, assemble)
        assert info["segments"] == 8
        if (n_reads, direct) == (150, "0"):
            assert info["fallbacks"] > 0           # the ladder runs on this form
        _same(got, want)
        if not assemble:
            assert int(want[0].max()) > 300        # an SFS per base of the longest insertions


# ---- f. heavy-first ordering on a rank-only table

def test_heavy_first_order_on_a_rank_only_table(monkeypatch):
    """1,200 reads and K = 9 >= 8: sfs_order_kernel sorts the reads by the table's estimate of their work."""
    ref, hap, svs, flat, offs = small_workload(seed=61, ref_lens=(300000, 120000), n_reads=1200, read_len=1500)
    ix, k = _resident(ref)
    assert k == 9
    want = O.OracleFMD.build(ref).search_batch(flat, offs, True)
    for order in (None, "0"):
        for seg in (None, "1"):
            for name, v in (("SVDSS_ORDER", order), ("SVDSS_SEGMENTS", seg)):
                if v is None:
                    monkeypatch.delenv(name, raising=False)
                else:
                    monkeypatch.setenv(name, v)
            got, info = _search(ix, flat, offs, True)
            if seg:
                assert info["segments"] == 1
            _same(got, want, (order, seg))
    assert want[0].sum() > 1200


# ---- g. knobs never change results

@pytest.mark.parametrize("knob,value", [("SVDSS_BS", "1"), ("SVDSS_SET", "0"), ("SVDSS_TABLE_FORWARD", "0"), ("SVDSS_TICKETS", "1"),
                                        ("SVDSS_BLOCKS", "1"), ("SVDSS_EXTRA_LDS", "32768")])
@pytest.mark.parametrize("seed", [31, 32])
def test_knobs_never_change_results(seed, knob, value, wide, monkeypatch, tmp_path_factory):
    """SVDSS_BS=1 asks for a kernel this form cannot run (no suffix array) and must be ignored; the others decide how
    the table is filled, how work is handed out and how many lanes are resident, never what is found."""
    monkeypatch.setenv(knob, value)
    ref, flat, offs, want, path = _case_b(seed, tmp_path_factory)
    ix = _open_resident(path, ref)             # (SVDSS_TABLE_FORWARD is read when the table is built)
    assert ix.kmer_k == 9
    for assemble in (False, True):
        for seg in (None, "1"):
            if seg:
                monkeypatch.setenv("SVDSS_SEGMENTS", seg)
            got, info = _search(ix, flat, offs, assemble)
            if seg:
                monkeypatch.delenv("SVDSS_SEGMENTS")
            assert info["bs"] is False
            assert (info["segments"] == 1) == (seg == "1")
            _same(got, want[assemble], (knob, assemble, seg))


def test_order_of_a_resident_handle_stays(monkeypatch, tmp_path_factory):
    ref, flat, offs, want, path = _case_b(32, tmp_path_factory)
    monkeypatch.setenv("SVDSS_LF_KMER", "6")
    ix = _open_resident(path, ref)
    assert ix.kmer_k == 6
    got, _ = _search(ix, flat, offs, True)
    _same(got, want[True])
    monkeypatch.setenv("SVDSS_LF_KMER", "3")
    got, _ = _search(ix, flat, offs, True)
    assert ix.kmer_k == 6
    _same(got, want[True])
    monkeypatch.delenv("SVDSS_LF_KMER")
    got, _ = _search(ix, flat, offs, False)
    assert ix.kmer_k == 6
    _same(got, want[False])


# ---- h. replicas

def _replica(src):
    h = C.c_void_p()
    check(lib.svdss_index_replicate(src._h, 0, C.byref(h)), "svdss_index_replicate")
    return svdss_amd.FMDIndex(h.value)


@pytest.mark.parametrize("source_resident", [False, True])
def test_replicas_of_a_rank_only_source(source_resident, wide, tmp_path_factory):
    """svdss_index_replicate uploads the blocks from the source's host copy and keeps none of its own: the replica
    searches, and answers what reads the index on the host with an error."""
    ref, flat, offs, want, path = _case_b(31, tmp_path_factory)
    src = R.open_rank_only(path)
    if source_resident:
        src.to_device(0)
        assert src.kmer_k == 9
    rep = _replica(src)
    assert rep.kmer_k == 9 and rep.size == src.size and (rep.acc == src.acc).all()
    assert R.records_code(rep) == R.ENODEV
    for assemble in (False, True):
        got, _ = _search(rep, flat, offs, assemble)
        _same(got, want[assemble])
    with pytest.raises(SvdssError) as err:
        rep.bwt()
    assert err.value.code == R.ENODEV
    assert rep.count(ref[0][10:30]) == -1
    rep.close()
    src.to_device(0)                             # the source still searches afterwards
    assert src.kmer_k == 9
    got, _ = _search(src, flat, offs, True)
    _same(got, want[True])


# ---- i. what a rank-only handle must refuse rather than crash on

def test_what_a_rank_only_handle_refuses(tmp_path, tmp_path_factory):
    ref, flat, offs, want, path = _case_b(31, tmp_path_factory)
    full = svdss_amd.FMDIndex.load(path)
    full.save_fmd(str(tmp_path / "full.fmd"))
    ix = _open_resident(path, ref)

    def code(fn, *a):
        with pytest.raises(SvdssError) as err:
            fn(*a)
        return err.value.code
    assert code(ix.verify) == R.EINVAL                                  # (nothing to verify against: no text)
    assert R.records_code(ix) == R.ENODEV
    assert code(ix.attach_blocks, path) == R.EINVAL                     # resident already
    assert code(ix.save, str(tmp_path / "a.svdss")) == R.ENODEV         # text and suffix array are nowhere
    assert code(ix.save_records, str(tmp_path / "b.svdss")) == R.ENODEV
    ix.save_fmd(str(tmp_path / "ro.fmd"))                               # the BWT is in the blocks
    assert (tmp_path / "ro.fmd").read_bytes() == (tmp_path / "full.fmd").read_bytes()
    got, _ = _search(ix, flat, offs, True)                              # ... and the handle still searches
    _same(got, want[True])


# ---- j. the production order

N_READS_K13 = 64      # (256 at first: see the test's docstring)

def test_production_order_13(monkeypatch, tmp_path):
    """K = 13, the order of every `run_svdss` search, at the smallest reference that has it: one contig of 33,600,000
    bases (n = 67,200,002 >= 4^13 = 67,108,864).  Index built in HBM and verified against its text, so that the oracle
    made of its BWT is an independent checker; reads of 3,000 bases from a haplotype with implanted SVs (0.5 % errors)
    and three exact reads, every read against the oracle, 32- and 64-bit intervals (one test for both: the index, its
    sidecar and the oracle's answers are made once).
    The one test of this file that is not a fraction of a second: 3.3 - 4.8 s on an MI355X machine with 256 reads, where
    test_scale_gpu.py::test_large_table_orders_match_oracle took 0.5 - 1.1 s; 2.6 s of it are the index build of the
    reference, which cannot be smaller, 0.4 s were the reads -- cut to 64 (N_READS_K13): 1.7 s, 1.3 s of them the build.
    The stage times are printed (pytest -s)."""
    import time
    n_ref, L, n_reads = 33_600_000, 3000, N_READS_K13
    t0, stages = time.perf_counter(), []

    def stage(name):
        stages.append(f"{name} {time.perf_counter() - t0:.2f}")
    ref = synth.make_reference([n_ref], seed=131)
    stage("reference")
    full = svdss_amd.FMDIndex.build(ref, device=0)
    stage("built")
    assert full.size == 2 * (n_ref + 1) >= 4 ** 13
    v = full.verify()
    assert v["rows"] == full.size and v["first_bad"] == -1, v
    assert v["bad_order"] == v["bad_bwt"] == v["bad_range"] == v["bad_block"] == v["bad_dollar"] == 0, v
    stage("verified")
    path = R.write_sidecar(full, str(tmp_path / "k13.svdss"))
    stage("sidecar")
    fm = O.OracleFMD.from_bwt(full.bwt())
    full.close()
    stage("oracle of the BWT")
    window = [ref[0][20_000_000:21_000_000]]
    hap, svs = synth.implant_svs(window, 8, seed=132)
    flat, offs, _ = synth.simulate_reads(hap, n_reads, L, 0.005, seed=133)
    reads = [flat[offs[i]:offs[i + 1]] for i in range(n_reads)]
    reads += [ref[0][n_ref - 20000:n_ref - 20000 + L].copy(), synth.revcomp(ref[0][5000:5000 + L]), ref[0][:L].copy()]
    flat, offs = svdss_amd.pack_reads(reads)
    want = {a: fm.search_batch(flat, offs, a) for a in (False, True)}
    stage("oracle's answers")
    assert want[False][0][:n_reads].sum() > n_reads and want[False][0][n_reads:].sum() == 0 and (want[False][3][n_reads:] == L - 1).all()
    for is_wide, lf_kmer in ((False, None), (True, None), (False, "14")):
        for name, v_ in (("SVDSS_FORCE_SA64", "1" if is_wide else None), ("SVDSS_LF_KMER", lf_kmer)):
            if v_ is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, v_)
        ix = R.open_rank_only(path).to_device(0)
        assert ix.kmer_k == 13 == R.expected_order(ref), (is_wide, lf_kmer)
        for assemble in (False, True):
            got, info = _search(ix, flat, offs, assemble)
            _same(got, want[assemble], (is_wide, lf_kmer, assemble))
            assert got.counts[n_reads:].sum() == 0 and (got.n_ext[n_reads:] == L - 1).all()
        ix.close()
        stage(f"searched (wide {is_wide}, SVDSS_LF_KMER {lf_kmer})")
    print("seconds since the start: " + ", ".join(stages))
