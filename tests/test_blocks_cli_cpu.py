"""The usage decisions of --blocks [--block-tol N] [--block-rows PATH] on check_graph, graph_simplifier and graph_builder --walk-pairs,
in the style of tests/test_judge_cli_cpu.py: all are made before a context is created, so no device is needed.  Each case runs a
tool in an empty directory and holds its exit code and the whole of stderr; nothing may reach stdout and no file may appear.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
B, S, K = "graph_builder", "graph_simplifier", "check_graph"
BIN = ["r.bin", "10", "31", "--walk-pairs", "2", "180", "250"]
GKG = ["g.gkg", "r.bin", "10", "--cutoff", "2"]
FASTA = ["--links", "l.tsv", "--scaffold-fasta", "s.fa"]
JUDGE = FASTA + ["--judge", "g.fa"]
CHK = ["g.gkg", "g.fa"]
WITH = "--blocks goes with --judge GENOME.fasta\n"
TOL_ALONE = "--block-tol N goes with --blocks\n"
ROWS_ALONE = "--block-rows PATH goes with --blocks\n"
NEG = "--block-tol N needs N >= 0\n"
K_USAGE = "usage: {exe} <graph.gkg> <genome.fasta> --blocks [--block-tol N] [--block-rows PATH]   (N defaults to 1000: a choice, not a measurement)\n"

# (tool, arguments, exit code, the whole of stderr)
CASES = [
    (S, GKG + ["--blocks"], 2, WITH),
    (S, GKG + FASTA + ["--blocks"], 2, WITH),
    (S, GKG + FASTA + ["--blocks", "--block-tol", "5"], 2, WITH),
    (S, GKG + JUDGE + ["--block-tol", "5"], 2, TOL_ALONE),
    (S, GKG + JUDGE + ["--block-rows", "rows.txt"], 2, ROWS_ALONE),
    (S, GKG + JUDGE + ["--blocks", "--block-tol", "-2"], 2, NEG),
    (S, GKG + JUDGE + ["--blocks", "--block-tol"], 2, "unknown argument --block-tol\n"),            # no value follows: the option took nothing
    (S, GKG + JUDGE + ["--blocks", "--block-rows"], 2, "unknown argument --block-rows\n"),
    (S, GKG + JUDGE + ["--blocks", "--world", "2", "--rank", "0", "--id-file", "id"], 2,
     "--links runs on one GPU only (not with --world): export per rank and add the tables\n"),
    (B, BIN + FASTA + ["--blocks"], 2, WITH),
    (B, BIN + JUDGE + ["--block-tol", "0"], 2, TOL_ALONE),
    (B, BIN + JUDGE + ["--block-rows", "rows.txt"], 2, ROWS_ALONE),
    (K, CHK + ["--block-tol", "5"], 2, TOL_ALONE + K_USAGE),
    (K, CHK + ["--block-rows", "rows.txt"], 2, ROWS_ALONE + K_USAGE),
    (K, CHK + ["--blocks", "--block-tol", "-2"], 2, NEG + K_USAGE),
    # past every usage decision: the first thing a run does is open its reads (the options before it were all taken)
    (S, GKG + JUDGE + ["--blocks"], 1, "graph_simplifier: cannot open r.bin\n"),
    (S, GKG + JUDGE + ["--judge-tol", "3", "--blocks", "--block-tol", "40", "--block-rows", "rows.txt"], 1, "graph_simplifier: cannot open r.bin\n"),
    (B, BIN + JUDGE + ["--blocks", "--block-tol", "0"], 1, "graph_builder: cannot open r.bin\n"),
]

# a value that is no integer: one line that names the option, exit 2
MALFORMED = [
    (S, GKG + JUDGE + ["--blocks", "--block-tol", "3x"], "--block-tol"),
    (B, BIN + JUDGE + ["--blocks", "--block-tol", "1.5"], "--block-tol"),
    (K, CHK + ["--blocks", "--block-tol", "99999999999999999999"], "--block-tol"),
]


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(HOST, t)) for t in (B, S, K)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return {t: os.path.join(HOST, t) for t in (B, S, K)}


def run(exe, args, cwd):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=30, cwd=cwd)
    assert r.stdout == "" and os.listdir(cwd) == [], (r.stdout, os.listdir(cwd))
    return r


@pytest.mark.parametrize("tool,args,code,stderr", CASES, ids=[f"{i}-{c[0]}-{'_'.join(c[1][-2:])}" for i, c in enumerate(CASES)])
def test_usage_decision(tools, tmp_path, tool, args, code, stderr):
    r = run(tools[tool], args, tmp_path)
    assert (r.returncode, r.stderr) == (code, stderr.format(exe=tools[tool]))


@pytest.mark.parametrize("tool,args,option", MALFORMED, ids=[f"{c[0]}-{c[2]}-{c[1][-1]}" for c in MALFORMED])
def test_malformed_number_names_the_option(tools, tmp_path, tool, args, option):
    r = run(tools[tool], args, tmp_path)
    assert r.returncode == 2 and r.stderr.startswith(option + " needs ") and r.stderr.count("\n") == 1 and args[-1] in r.stderr, r.stderr


def test_the_help_text_says_the_default(tools, tmp_path):
    """tol is a choice: every tool's usage text names the default"""
    for t in (B, S):
        r = run(tools[t], [], tmp_path)
        assert r.returncode == 2 and "[--blocks [--block-tol N (default 1000: a choice, not a measurement)] [--block-rows PATH]]" in r.stderr
    r = run(tools[K], CHK + ["--block-tol", "7"], tmp_path)
    assert "N defaults to 1000: a choice, not a measurement" in r.stderr
