"""The usage decisions of --resolve-repeats [CUTOFF] [--resolve-rounds N] on graph_simplifier and graph_builder --walk-pairs, in the
style of tests/test_host_cli_cpu.py: all are made before a context is created, so no device is needed.  Each case runs a tool in
an empty directory and holds its exit code and the whole of stderr; nothing may reach stdout and no file may appear.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
B, S = "graph_builder", "graph_simplifier"
WORLD = ["--world", "2", "--rank", "0", "--id-file", "id"]
BIN = ["r.bin", "10", "31", "--walk-pairs", "2", "180", "250"]
GKG = ["g.gkg", "r.bin", "10", "--cutoff", "2"]
CUTOFF = "--resolve-repeats CUTOFF is 1..4294967295\n"
ROUNDS = "--resolve-rounds N needs N >= 1\n"
ALONE = "--resolve-rounds N goes with --resolve-repeats\n"
ONE_GPU = "--resolve-repeats runs on one GPU only (not with --world): the spans have no collective\n"
NO_PAIRS = "--no-pairs goes with --thread-reads, and not with --range auto (no walk uses the range)\n"

# (tool, arguments, exit code, the whole of stderr)
CASES = [
    (S, GKG + ["--resolve-repeats", "0"], 2, CUTOFF),
    (S, GKG + ["--resolve-repeats", "4294967296"], 2, CUTOFF),
    (S, GKG + ["--resolve-repeats", "--resolve-rounds", "0"], 2, ROUNDS),
    (S, GKG + ["--resolve-rounds", "2"], 2, ALONE),
    (S, GKG + ["--resolve-repeats", "--resolve-rounds"], 2, "unknown argument --resolve-rounds\n"),
    (S, GKG + ["--resolve-repeats", "x3"], 2, "unknown argument x3\n"),           # no number follows: the option took nothing
    (S, GKG + ["--resolve-repeats"] + WORLD, 2, ONE_GPU),
    (S, GKG + ["--resolve-repeats", "--no-pairs", "--range", "auto"], 2, NO_PAIRS),
    (B, BIN + ["--resolve-repeats", "0"], 2, CUTOFF),
    (B, BIN + ["--resolve-repeats", "3", "--resolve-rounds", "0"], 2, ROUNDS),
    (B, BIN + ["--resolve-rounds", "2"], 2, ALONE),
    (B, BIN + ["--resolve-repeats"] + WORLD, 2, ONE_GPU),
    (B, ["r.bin", "10", "31", "--resolve-repeats"], 2, "--resolve-repeats goes with --walk-pairs (it runs behind the paired-end stage)\n"),
    # past every usage decision: the first thing a run does is open its reads (the options before it were all taken)
    (S, GKG + ["--no-pairs", "--resolve-repeats"], 1, "graph_simplifier: cannot open r.bin\n"),
    (S, GKG + ["--thread-reads", "--resolve-repeats", "3", "--resolve-rounds", "4", "--contigs", "c.fa"], 1, "graph_simplifier: cannot open r.bin\n"),
    (B, BIN + ["--resolve-repeats", "--resolve-rounds", "2"], 1, "graph_builder: cannot open r.bin\n"),
]

# a value that is no number of the option's kind: one line that names the option, exit 2
MALFORMED = [
    (S, GKG + ["--resolve-repeats", "3x"], "--resolve-repeats"),
    (S, GKG + ["--resolve-repeats", "99999999999999999999"], "--resolve-repeats"),
    (S, GKG + ["--resolve-repeats", "--resolve-rounds", "x"], "--resolve-rounds"),
    (S, GKG + ["--resolve-repeats", "--resolve-rounds", "-1"], "--resolve-rounds"),
    (B, BIN + ["--resolve-repeats", "3x"], "--resolve-repeats"),
    (B, BIN + ["--resolve-repeats", "--resolve-rounds", "1.5"], "--resolve-rounds"),
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


@pytest.mark.parametrize("tool,args,code,stderr", CASES, ids=[f"{c[0]}-{'_'.join(c[1][-3:])}" for c in CASES])
def test_usage_decision(tools, tmp_path, tool, args, code, stderr):
    r = run(tools[tool], args, tmp_path)
    assert (r.returncode, r.stderr) == (code, stderr)


@pytest.mark.parametrize("tool,args,option", MALFORMED, ids=[f"{c[0]}-{c[2]}-{c[1][-1]}" for c in MALFORMED])
def test_malformed_number_names_the_option(tools, tmp_path, tool, args, option):
    r = run(tools[tool], args, tmp_path)
    assert r.returncode == 2 and r.stderr.startswith(option + " needs ") and r.stderr.count("\n") == 1 and args[-1] in r.stderr, r.stderr
