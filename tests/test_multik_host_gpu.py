"""graph_builder --seed-k (the C++ tool, genome::DNAMap::addGraphPaths behind it) on the construction of tests/multik_cases.py: the
seeded k = 55 run writes the genome as one record where the plain run writes two, its "seed_stages" carry the numbers
genome_amd.multik.assemble reports, and the option's usage errors.  -m gpu."""
import json
import os
import subprocess

import pytest

import multik_cases as MC
from genome_amd import dna
from genome_amd.dnamap import Context
from genome_amd.multik import assemble
from oracle import pyref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDER = os.path.join(ROOT, "genome_amd", "host", "graph_builder")


def run(args):
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


def records(path):
    return ["".join(r.split("\n")[1:]) for r in open(path).read().split(">") if r]


@pytest.mark.parametrize("form", ["bin", "fastq"])
def test_seeded_builder_writes_the_genome_as_one_record(tmp_path, form):
    genome = MC.dip_genome()
    reads = MC.dip_reads(genome)
    if form == "bin":
        (tmp_path / "r.bin").write_bytes(dna.reads_to_bin(reads))
        base = [BUILDER, tmp_path / "r.bin", len(reads) // 2, 55]
    else:
        (tmp_path / "r.fastq").write_text("".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads)))
        base = [BUILDER, "--fastq", tmp_path / "r.fastq", 55, "--interleaved"]
    base += ["--no-retain", "--simplify", "--contigs"]
    js, err = run(base + [tmp_path / "seeded.fa", "--seed-k", 21])
    assert records(tmp_path / "seeded.fa") in ([genome], [R.rev_comp(genome)])
    if form == "fastq":
        return
    js0, err0 = run(base + [tmp_path / "plain.fa"])
    assert len(records(tmp_path / "plain.fa")) == 2 and "seed_stages" not in js0 and "seed-k" not in err0
    # the same numbers as Python's driver, stage by stage, and one line per stage on stderr
    ctx = Context(0)
    m, g, stages = assemble(ctx, dna.reads_to_bin(reads), len(reads), [21, 55])
    g.close(); m.close(); ctx.close()
    assert js["seed_stages"] == stages
    assert js["seed_stages"][1]["windows"] == len(genome) - 55 + 1 and js["seed_stages"][1]["forward"] == 1
    assert [x.split()[2] for x in err.splitlines() if x.startswith("seed-k: k ")] == ["21", "55"]


@pytest.mark.parametrize("extra, message", [
    (["--seed-k", "31,21"], "usage: --seed-k"),
    (["--seed-k", "32"], "usage: --seed-k"),
    (["--seed-k", "55"], "usage: --seed-k"),
    (["--seed-k", "21,x"], "usage: --seed-k"),
    (["--seed-k", "21", "--world", "2", "--rank", "0", "--id-file", "id"], "--seed-k runs on one GPU only (not with --world)"),
    (["--seed-k", "21", "--prefilter", "1000"], "--seed-k does not run with --prefilter"),
])
def test_seed_k_usage_errors(extra, message):
    r = subprocess.run([BUILDER, "r.bin", "10", "55"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr and r.stdout == ""
