"""`SVDSS run --samples LIST` on the command line (csrc/run_samples.h, csrc/cli_options.h, csrc/svdss_main.cpp,
csrc/run_host.cpp): the list parser against a restatement of its rules in Python, and every refusal -- each said before
anything is opened for writing and before the GPU is looked for, so none of this needs one."""
import os
import random
import subprocess

import pytest

from tests import bam_writer
from tests.common import BIN, ROOT

KNOBS = ("SVDSS_INDEX_CPU", "SVDSS_SMOOTH_HOST", "SVDSS_BAM_DEVICE", "SVDSS_GPU_DEFLATE")
PARSE_SRC = os.path.join(ROOT, "tests", "native", "run_samples_parse.cpp")
PARSE_EXE = os.path.join(ROOT, "tests", "native", "_run_samples_parse")


def run(*args, env=None, cwd=None):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS} if env is None else env
    return subprocess.run([BIN, *map(str, args)], capture_output=True, timeout=120, env=env, cwd=cwd)


@pytest.fixture(scope="module")
def exe():
    hdr = os.path.join(ROOT, "svdss_amd", "csrc", "run_samples.h")
    if not os.path.exists(PARSE_EXE) or os.path.getmtime(PARSE_EXE) < max(os.path.getmtime(PARSE_SRC), os.path.getmtime(hdr)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-o", PARSE_EXE, PARSE_SRC], check=True)
    return PARSE_EXE


# ---------------------------------------------------------------- the parser

def parse_py(data, inputs, list_name):
    """The rules of csrc/run_samples.h, restated: (samples, None) or (None, the key words of the refusal)."""
    samples = []
    for n, line in enumerate(data.split(b"\n"), 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line.startswith(b"#"):
            continue
        cols = line.split(b"\t")
        if len(cols) < 2:
            return None, (n, "fewer than two")
        if len(cols) > 3:
            return None, (n, "more than three")
        for k, c in enumerate(cols):
            if not c:
                return None, (n, f"column {k + 1} is empty")
        samples.append((n, cols[0], cols[1], cols[2] if len(cols) == 3 else b""))
    if not samples:
        return None, (None, "no sample in the list")
    reads = set(inputs) | {list_name} | {s[1] for s in samples}
    writes = set()
    for n, _, vcf, sfs in samples:
        for p in (vcf, sfs):
            if not p:
                continue
            if p in reads:
                return None, (n, "is an input of the run")
            if p in writes:
                return None, (n, "is named twice")
            writes.add(p)
    return samples, None


def generated_lists():
    rng = random.Random(11)
    names = [b"a.bam", b"b.bam", b"dir with spaces/c d.bam", b"a.vcf", b"b.vcf", b"out dir/c.vcf", b"a.sfs", b"b.sfs", b" lead.vcf", b"trail.vcf ",
             b"ref.fa", b"ref.fa.fmd", b"#not-a-comment.vcf"]
    lists = [b"", b"\n\n# only a comment\n", b"a.bam\ta.vcf", b"a.bam\ta.vcf\n", b"a.bam\ta.vcf\r\nb.bam\tb.vcf\tb.sfs\r\n", b"a.bam\ta.vcf\t\n",
             b"a.bam\ta.vcf\ta.sfs\t\n", b"a.bam\n", b"a.bam\t\ta.sfs\n", b"\ta.vcf\n", b"a.bam\ta.vcf\nb.bam\ta.vcf\n", b"a.bam\ta.vcf\ta.vcf\n",
             b"a.bam\tb.bam\nb.bam\tb.vcf\n", b"a.bam\tref.fa\n", b"a.bam\ta.vcf\tref.fa.fmd\n", b"a.bam\ta.vcf\na.bam\tb.vcf\n", b" \n", b"a.bam a.vcf\n",
             b"a.bam\ta.vcf\n\r\n#x\ty\n\nb.bam\tb.vcf", b"a.bam\tLIST\n", b"a.bam\ta.vcf\r\r\n"]
    for _ in range(40):
        lines = []
        for _ in range(rng.randint(1, 6)):
            kind = rng.random()
            if kind < 0.15:
                lines.append(rng.choice([b"", b"# a comment\twith a tab", b"#", b"\r"[:0]]))
                continue
            cols = [rng.choice(names) for _ in range(rng.choice([2, 2, 3, 3, 3, 1, 4]))]
            line = b"\t".join(cols)
            if rng.random() < 0.1:
                line += b"\t"
            lines.append(line)
        end = rng.choice([b"\n", b"\r\n"])
        data = end.join(lines) + (end if rng.random() < 0.7 else b"")
        lists.append(data)
    return lists


def test_parser_against_its_restatement(exe, tmp_path):
    inputs = [b"ref.fa", b"ref.fa.fmd"]
    n_ok = n_refused = 0
    seen = set()
    for k, data in enumerate(generated_lists()):
        path = tmp_path / f"list{k}.txt"
        data = data.replace(b"LIST", str(path).encode())
        path.write_bytes(data)
        want, why = parse_py(data, inputs, str(path).encode())
        r = subprocess.run([exe, str(path), *[i.decode() for i in inputs]], capture_output=True, timeout=60)
        if want is None:
            n_refused += 1
            seen.add(why[1])
            assert r.returncode == 1 and r.stdout == b"", (data, r.stdout, r.stderr)
            assert why[1].encode() in r.stderr and str(path).encode() in r.stderr, (data, why, r.stderr)
            if why[0] is not None:
                assert b" line %d: " % why[0] in r.stderr, (data, why, r.stderr)
        else:
            n_ok += 1
            assert r.returncode == 0, (data, r.stderr)
            got = [tuple(l.split(b"\t")) for l in r.stdout.split(b"\n")[:-1]]
            assert got == [(str(n).encode(), b, v, s) for n, b, v, s in want], (data, r.stdout)
    print(n_ok, "lists parsed,", n_refused, "refused:", sorted(seen))
    assert n_ok >= 10 and n_refused >= 20
    assert seen >= {"fewer than two", "more than three", "column 1 is empty", "column 2 is empty", "column 3 is empty", "no sample in the list",
                    "is an input of the run", "is named twice"}
    r = subprocess.run([exe, str(tmp_path / "absent.txt")], capture_output=True, timeout=60)
    assert r.returncode == 1 and b"cannot read the list" in r.stderr


# ---------------------------------------------------------------- the refusals of the binary

@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("samples_cli")
    fa = tmp / "r.fa"
    fa.write_text(">c\n" + "ACGT" * 500 + "\n")
    bams = []
    for k in range(2):
        bam = tmp / f"x{k}.bam"
        bam.write_bytes(bam_writer.bam([("c", 2000)], [bam_writer.record("q", 0, 0, 10, 60, [("M", 100)], "ACGT" * 25)]))
        bams.append(bam)
    fmd = tmp / "r.fa.fmd"
    fmd.write_bytes(b"not read before the refusals")
    return {"tmp": tmp, "fa": fa, "bams": bams, "fmd": fmd}


def outputs(tmp):
    return sorted(p.name for p in tmp.iterdir() if p.suffix in (".vcf", ".sfs", ".tmp", ".sam", ".bai", ".txt") and not p.name.startswith("list"))


def refused(fx, list_text, word, *more, cmd="run", env=None):
    tmp = fx["tmp"]
    lst = tmp / "list.txt"
    if list_text is not None:
        lst.write_bytes(list_text.encode() if isinstance(list_text, str) else list_text)
    elif lst.exists():
        lst.unlink()
    before = outputs(tmp)
    r = run(cmd, "--reference", fx["fa"], "--index", fx["fmd"], "--samples", lst, *more, env=env)
    assert r.returncode == 1, (word, r.stderr)
    assert word.encode() in r.stderr, (word, r.stderr)
    assert r.stdout == b""
    assert outputs(tmp) == before == [], (word, outputs(tmp))
    return r


def two(fx):
    t = fx["tmp"]
    return f"{fx['bams'][0]}\t{t}/o0.vcf\t{t}/o0.sfs\n{fx['bams'][1]}\t{t}/o1.vcf\n"


@pytest.mark.parametrize("opt", ["--bam", "--sfs", "--smoothed", "--write-index", "--compress", "--poa", "--clusters"])
def test_options_samples_does_not_go_with(fx, opt):
    value = {"--bam": fx["bams"][0], "--compress": "runs"}.get(opt, fx["tmp"] / "side.txt")
    r = refused(fx, two(fx), "--samples does not go with " + opt, opt, value)
    assert b"critical" in r.stderr


@pytest.mark.parametrize("cmd", ["smooth", "search", "call"])
def test_samples_is_runs_alone(fx, cmd):
    refused(fx, two(fx), "--samples is an option of `SVDSS run` only, not of `SVDSS " + cmd + "`", "--bam", fx["bams"][0], "--sfs", fx["tmp"] / "x.sfs", cmd=cmd)


def test_list_that_cannot_be_read(fx):
    refused(fx, None, "cannot read the list")


@pytest.mark.parametrize("text", ["", "\n# nothing\n\r\n"])
def test_list_without_a_sample(fx, text):
    refused(fx, text, "no sample in the list")


def test_malformed_lines(fx):
    b, t = fx["bams"][0], fx["tmp"]
    refused(fx, f"# ok\n{b}\n", "line 2: fewer than two")
    refused(fx, f"{b}\t{t}/a.vcf\t{t}/a.sfs\t{t}/more\n", "line 1: more than three")
    refused(fx, f"{b}\t{t}/a.vcf\n{b}\t\t{t}/a.sfs\n", "line 2: column 2 is empty")
    refused(fx, f"{b}\t{t}/a.vcf\t\n", "line 1: column 3 is empty")
    refused(fx, f"\t{t}/a.vcf\n", "line 1: column 1 is empty")


def test_bam_that_does_not_exist(fx):
    t = fx["tmp"]
    refused(fx, f"{fx['bams'][0]}\t{t}/a.vcf\n{t}/absent.bam\t{t}/b.vcf\n", f"line 2: cannot read {t}/absent.bam")


def test_same_output_twice(fx):
    b, t = fx["bams"], fx["tmp"]
    refused(fx, f"{b[0]}\t{t}/a.vcf\n{b[1]}\t{t}/a.vcf\n", "line 2: the output " + f"{t}/a.vcf is named twice")
    refused(fx, f"{b[0]}\t{t}/a.vcf\t{t}/a.vcf\n", "is named twice")
    refused(fx, f"{b[0]}\t{t}/a.vcf\t{t}/a.sfs\n{b[1]}\t{t}/b.vcf\t{t}/a.sfs\n", "line 2: the output " + f"{t}/a.sfs is named twice")


def test_output_that_is_an_input(fx):
    b, t = fx["bams"], fx["tmp"]
    refused(fx, f"{b[0]}\t{b[1]}\n{b[1]}\t{t}/b.vcf\n", f"line 1: the output {b[1]} is an input of the run")
    refused(fx, f"{b[0]}\t{t}/a.vcf\t{fx['fa']}\n", "is an input of the run")
    refused(fx, f"{b[0]}\t{fx['fmd']}\n", "is an input of the run")
    refused(fx, f"{b[0]}\t{t}/list.txt\n", "is an input of the run")
    refused(fx, f"{b[0]}\t{t}/./r.fa\n", "is an input of the run")          # another spelling of the FASTA's path
    for p in b + [fx["fa"], fx["fmd"]]:
        assert p.stat().st_size > 0


def test_what_run_refuses_stays_refused(fx):
    refused(fx, two(fx), "out of scope", "--gpus", "2")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    refused(fx, two(fx), "SVDSS_SMOOTH_HOST", env=dict(env, SVDSS_SMOOTH_HOST="1"))
    refused(fx, two(fx), "SVDSS_BAM_DEVICE", env=dict(env, SVDSS_BAM_DEVICE="0"))
    r = run("run", "--reference", fx["fa"], "--samples", fx["tmp"] / "list.txt")        # no --index
    assert r.returncode == 1 and b"Usage: SVDSS run" in r.stderr and r.stdout == b""


def test_usage_names_the_option():
    r = run("run", "--help")
    assert r.returncode == 0 and b"--samples <LIST>" in r.stderr and b"BAM<TAB>VCF[<TAB>SFS]" in r.stderr and r.stdout == b""


def test_good_list_fails_loudly_without_a_gpu(fx):
    import torch
    if torch.cuda.is_available():
        pytest.skip("this machine has a GPU")
    refused(fx, two(fx), "no GPU found")
