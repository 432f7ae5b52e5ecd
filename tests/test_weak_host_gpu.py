"""graph_builder --remove-weak end to end on the GPU (-m gpu), on the planted read set of tests/weak_planted.py (checked on the CPU
in tests/test_weak_cpu.py): the bridge goes in round 1 and the two segments come out as two contigs per strand; without the flag
the very bytes the parent commit wrote (tests/golden/weak/parent_hashes.json: sha256 of stdout and of every output file, recorded
with the parent's build before the flag existed); with --world exit 2."""
import hashlib
import json
import os
import subprocess

import pytest

from genome_amd import dna
from oracle import pyref as R

import weak_planted as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "genome_amd", "host", "graph_builder")
PARENT_RUNS = {"clean": ["--no-retain", "--clip-tips", "--pop-bubbles"], "clean_simplify": ["--clip-tips", "--pop-bubbles", "--simplify"]}


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return EXE


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    binb = dna.reads_to_bin(P.reads())
    path = tmp_path_factory.mktemp("weak") / "reads.bin"
    path.write_bytes(binb)
    return binb, str(path)


def command(exe, binf, *flags):
    return [exe, binf, str(len(P.reads()) // 2), str(P.K), "--rounds", str(P.ROUNDS), *flags]


def run(exe, binf, *flags):
    res = subprocess.run(command(exe, binf, *flags), capture_output=True)
    assert res.returncode == 0, res.stderr.decode()
    return res


def path_edge(p):
    return [p[:P.K], p[-P.K:], p[P.K:]]


def test_the_planted_bridge_goes_in_round_one(exe, reads, tmp_path):
    _binb, binf = reads
    out = str(tmp_path / "w")
    res = run(exe, binf, "--no-retain", "--clip-tips", "--pop-bubbles", "--remove-weak", "--out", out)
    stats = json.loads(res.stdout)
    assert stats["remove_weak"] == {"max_len": 2 * P.K, "ratio": 5, "floor": 0, "candidates": [2, 0], "removed_ratio": [2, 0], "removed_floor": [0, 0]}
    assert stats["clip_tips"]["removed"] == [0, 0] and stats["pop_bubbles"]["removed"] == [0, 0]
    assert b"remove-weak: 2 edges by ratio 5" in res.stderr
    # the two segments, one contig per strand each
    s1, s2 = P.segments()
    want = sorted(path_edge(p) for s in (s1, s2) for p in (s, R.rev_comp(s)))
    assert sorted(line.split() for line in open(out + ".edges.txt").read().splitlines()) == want
    assert (stats["graph_edges"], stats["retained_edges"]) == (10, 4)
    # the explicit forms of the options give the same run
    again = json.loads(run(exe, binf, "--no-retain", "--clip-tips", "--pop-bubbles", "--remove-weak", "5", "--weak-max-len", str(2 * P.K), "--min-coverage", "0").stdout)
    assert again == stats
    # without --remove-weak the bridge stays: more edges, and no trace of the option
    plain = json.loads(run(exe, binf, "--no-retain", "--clip-tips", "--pop-bubbles").stdout)
    assert plain["retained_edges"] == 10 > stats["retained_edges"] and "remove_weak" not in plain
    # the ratio rule off and a floor between the bridge's mean (8.8) and the segments' (about 56): the floor alone takes it
    floor = json.loads(run(exe, binf, "--no-retain", "--remove-weak", "0", "--min-coverage", "20").stdout)
    assert floor["remove_weak"] == {"max_len": 2 * P.K, "ratio": 0, "floor": 20, "candidates": [2, 0], "removed_ratio": [0, 0], "removed_floor": [2, 0]}
    assert floor["retained_edges"] == 4


@pytest.mark.parametrize("name", sorted(PARENT_RUNS))
def test_without_the_flag_every_output_is_the_parents(exe, reads, tmp_path, name):
    binb, binf = reads
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "weak", "parent_hashes.json")))
    assert hashlib.sha256(binb).hexdigest() == golden["reads_sha256"]
    out = str(tmp_path / name)
    res = run(exe, binf, *PARENT_RUNS[name], "--out", out)
    got = {"stdout": hashlib.sha256(res.stdout).hexdigest()}
    for ext in (".nodes.txt", ".edges.txt", ".contigs", ".dot"):
        got[ext] = hashlib.sha256(open(out + ext, "rb").read()).hexdigest()
    assert got == golden[name]
    assert b"remove-weak" not in res.stderr and b"remove_weak" not in res.stdout


def test_remove_weak_does_not_run_over_ranks_and_checks_its_values(exe, reads, tmp_path):
    _binb, binf = reads
    res = subprocess.run(command(exe, binf, "--remove-weak", "--world", "2", "--rank", "0", "--id-file", str(tmp_path / "id")), capture_output=True)
    assert res.returncode == 2 and b"--remove-weak" in res.stderr
    assert subprocess.run(command(exe, binf, "--remove-weak", "65536"), capture_output=True).returncode == 2
    res = subprocess.run(command(exe, binf, "--min-coverage", "3"), capture_output=True)               # only with --remove-weak
    assert res.returncode == 2 and b"--min-coverage" in res.stderr
