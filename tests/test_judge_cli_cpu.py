"""The usage decisions of --judge GENOME.fasta [--judge-tol N] on graph_simplifier and graph_builder --walk-pairs, in the style of
tests/test_spans_cli_cpu.py: all are made before a context is created, so no device is needed.  Each case runs a tool in an empty
directory and holds its exit code and the whole of stderr; nothing may reach stdout and no file may appear.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
B, S = "graph_builder", "graph_simplifier"
BIN = ["r.bin", "10", "31", "--walk-pairs", "2", "180", "250"]
GKG = ["g.gkg", "r.bin", "10", "--cutoff", "2"]
LINKS = ["--links", "l.tsv"]
FASTA = LINKS + ["--scaffold-fasta", "s.fa"]
WITH = "--judge GENOME.fasta goes with --scaffold-fasta PATH\n"
ALONE = "--judge-tol N goes with --judge GENOME.fasta\n"

# (tool, arguments, exit code, the whole of stderr)
CASES = [
    (S, GKG + ["--judge", "g.fa"], 2, WITH),
    (S, GKG + LINKS + ["--judge", "g.fa"], 2, WITH),
    (S, GKG + LINKS + ["--scaffolds", "s.txt", "--judge", "g.fa"], 2, WITH),          # the id list is no plan
    (S, GKG + FASTA + ["--judge-tol", "5"], 2, ALONE),
    (S, GKG + FASTA + ["--judge"], 2, "unknown argument --judge\n"),                  # no value follows: the option took nothing
    (S, GKG + FASTA + ["--judge", "g.fa", "--judge-tol"], 2, "unknown argument --judge-tol\n"),
    (S, GKG + FASTA + ["--judge", "g.fa", "--judge-tol", "-2"], 2, "--judge-tol N needs N >= 0\n"),
    (S, GKG + FASTA + ["--judge", "g.fa", "--world", "2", "--rank", "0", "--id-file", "id"], 2,
     "--links runs on one GPU only (not with --world): export per rank and add the tables\n"),
    (B, BIN + ["--judge", "g.fa"], 2, WITH),
    (B, BIN + LINKS + ["--judge", "g.fa"], 2, WITH),
    (B, BIN + FASTA + ["--judge-tol", "0"], 2, ALONE),
    # past every usage decision: the first thing a run does is open its reads (the options before it were all taken)
    (S, GKG + FASTA + ["--judge", "g.fa"], 1, "graph_simplifier: cannot open r.bin\n"),
    (S, GKG + FASTA + ["--judge", "g.fa", "--judge-tol", "0", "--overlap-gaps"], 1, "graph_simplifier: cannot open r.bin\n"),
    (B, BIN + FASTA + ["--judge", "g.fa", "--judge-tol", "35"], 1, "graph_builder: cannot open r.bin\n"),
]

# a value that is no integer: one line that names the option, exit 2
MALFORMED = [
    (S, GKG + FASTA + ["--judge", "g.fa", "--judge-tol", "3x"], "--judge-tol"),
    (S, GKG + FASTA + ["--judge", "g.fa", "--judge-tol", "1.5"], "--judge-tol"),
    (B, BIN + FASTA + ["--judge", "g.fa", "--judge-tol", "99999999999999999999"], "--judge-tol"),
]


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(HOST, t)) for t in (B, S)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return {t: os.path.join(HOST, t) for t in (B, S)}


def run(exe, args, cwd):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=30, cwd=cwd)
    assert r.stdout == "" and os.listdir(cwd) == [], (r.stdout, os.listdir(cwd))
    return r


@pytest.mark.parametrize("tool,args,code,stderr", CASES, ids=[f"{i}-{c[0]}-{'_'.join(c[1][-2:])}" for i, c in enumerate(CASES)])
def test_usage_decision(tools, tmp_path, tool, args, code, stderr):
    r = run(tools[tool], args, tmp_path)
    assert (r.returncode, r.stderr) == (code, stderr)


@pytest.mark.parametrize("tool,args,option", MALFORMED, ids=[f"{c[0]}-{c[2]}-{c[1][-1]}" for c in MALFORMED])
def test_malformed_number_names_the_option(tools, tmp_path, tool, args, option):
    r = run(tools[tool], args, tmp_path)
    assert r.returncode == 2 and r.stderr.startswith(option + " needs ") and r.stderr.count("\n") == 1 and args[-1] in r.stderr, r.stderr
