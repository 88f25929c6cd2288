"""`SVDSS index -i OLD` on the GPU box: the records of an index without a sidecar recovered by the device walk
(csrc/bwt_invert.hip), the new index built in HBM -- the same bytes as the index of the concatenated inputs -- and
`search --fastx` writes the same text against the appended index from every route."""
import os

import pytest

from svdss_amd import synth
from tests import index_append_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("append_gpu")
    a, b = A.make_inputs(d)
    A.index(d, "-d", d / "ab.fa", "-o", d / "ab.fmd")
    A.index(d, "-d", d / "a.fa", "-o", d / "a.fmd")
    hap, _ = synth.implant_svs((a + b)[:2] + b[:1], 3, seed=33, min_len=30, max_len=120)
    flat, offs, _ = synth.simulate_reads(hap, 300, 150, 0.01, seed=34)
    with open(d / "reads.fq", "w") as fh:
        for i in range(len(offs) - 1):
            s = synth.to_ascii(flat[offs[i]:offs[i + 1]])
            fh.write(f"@r{i}\n{s}\n+\n{'I' * len(s)}\n")
    return d, a, b, A.pair(d / "ab.fmd")


def search(d, fmd):
    r = A.run("search", "--index", str(fmd), "--fastx", str(d / "reads.fq"), "--threads", "4")
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout


def test_append_through_the_gpu_builder_and_the_device_walk(case, tmp_path):
    d, a, b, want = case
    text = search(d, d / "ab.fmd")
    assert text.count(b"\n") > 20
    routes = {}
    # several inputs; the sidecar
    A.index(d, "-d", d / "a.fa", d / "b.fa.gz", "-o", tmp_path / "x.fmd")
    A.index(d, "-i", d / "a.fmd", "-d", d / "b.fa.gz", "-o", tmp_path / "side.fmd")
    # an index in ropebwt's order without a sidecar: the device walk
    A.rope_fmd(a, tmp_path / "up.fmd")
    r = A.index(d, "-i", tmp_path / "up.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "walk.fmd")
    err = r.stderr.decode()
    assert "from its BWT by the device walk (stride 1024" in err and "pass 2" in err, err
    for name in ("x", "side", "walk"):
        assert A.pair(tmp_path / f"{name}.fmd") == want, name
        routes[name] = tmp_path / f"{name}.fmd"
    # SVDSS_FMD_IMPORT_DEVICE=0: the serial host walk, the same bytes
    r = A.index(d, "-i", tmp_path / "up.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "host.fmd",
                env=dict(os.environ, SVDSS_FMD_IMPORT_DEVICE="0"))
    assert "one serial walk per string" in r.stderr.decode() and A.pair(tmp_path / "host.fmd") == want
    # this library's own .fmd with its sidecar gone: another record order, the same answers
    (tmp_path / "a.fmd").write_bytes((d / "a.fmd").read_bytes())
    r = A.index(d, "-i", tmp_path / "a.fmd", "--verbose", "-d", d / "b.fa.gz", "-o", tmp_path / "own.fmd")
    assert "device walk" in r.stderr.decode()
    routes["own"] = tmp_path / "own.fmd"
    for name, fmd in routes.items():
        assert search(d, fmd) == text, name


def test_search_imports_an_fmd_by_the_device_walk_when_asked(case, tmp_path):
    """SVDSS_FMD_IMPORT_DEVICE=1: `search --index upstream.fmd` recovers the records on the GPU; the same text"""
    d, a, b, want = case
    A.rope_fmd(a + b, tmp_path / "up_ab.fmd")
    text = search(d, d / "ab.fmd")
    r = A.run("search", "--index", str(tmp_path / "up_ab.fmd"), "--fastx", str(d / "reads.fq"), "--threads", "4",
              env=dict(os.environ, SVDSS_FMD_IMPORT_DEVICE="1"))
    assert r.returncode == 0 and r.stdout == text, r.stderr.decode()
    assert search(d, tmp_path / "up_ab.fmd") == text
