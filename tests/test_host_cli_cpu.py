"""The usage decisions of the five C++ tools (genome_amd/host), which are all made before a context is created: no device needed.
Each case runs a tool in an empty directory and holds its exit code and stderr to literals recorded from the tools as they were
before tool_common.hpp (the malformed-number cases excepted: those ended in std::terminate, and are usage errors now); nothing
may reach stdout and no file may appear.  And tests/host/tool_common_check.cpp, the header's device-free parts as a program of
its own under AddressSanitizer and UndefinedBehaviorSanitizer (the model: tests/test_scratch_cpu.py).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "genome_amd", "host")
TOOLS = ("graph_builder", "graph_simplifier", "correct_reads", "check_graph", "convert2bin")
B, S, C, K, V = TOOLS

BUILDER_FASTQ_USAGE = ("usage: {exe} --fastq <reads.fastq> <k> [--split N | --interleaved] [options of the .bin form]\n"
                       "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n")
SIMPLIFIER_FASTQ_USAGE = ("usage: {exe} <graph.gkg> --fastq <reads.fastq> --cutoff C [--split N | --interleaved] [options of the .bin form]\n"
                          "       (--fastq takes --split N or --interleaved; it does not run with --world: convert2bin first)\n")
WORLD = ["--world", "2", "--rank", "0", "--id-file", "id"]
ONE_GPU = " on one GPU only (not with --world)\n"
BIN = ["r.bin", "10", "31"]                   # graph_builder's and correct_reads' positionals
GKG = ["g.gkg", "r.bin", "10"]                # graph_simplifier's
MAX_INSERT = "--max-insert N is 1..65535; --insert-hist PATH goes with --range auto\n"
NO_PAIRS = "--no-pairs goes with --thread-reads, and not with --range auto (no walk uses the range)\n"

# (tool, arguments, exit code, the whole of stderr; {exe} = the tool's path as it was called)
CASES = [
    (B, BIN + ["--bogus"], 2, "unknown argument --bogus\n"),
    (B, BIN + ["--out"], 2, "unknown argument --out\n"),
    (B, BIN + ["--world", "2"], 2, "--world W needs --rank R (0 <= R < W) and --id-file PATH\n"),
    (B, BIN + WORLD + ["--prefilter", "1"], 2, "--prefilter runs" + ONE_GPU),
    (B, BIN + WORLD + ["--clip-tips"], 2, "--clip-tips and --edge-coverage run" + ONE_GPU),
    (B, BIN + WORLD + ["--edge-coverage"], 2, "--clip-tips and --edge-coverage run" + ONE_GPU),
    (B, BIN + WORLD + ["--correct", "auto"], 2, "--correct runs" + ONE_GPU),
    (B, BIN + WORLD + ["--pop-bubbles"], 2, "--pop-bubbles runs" + ONE_GPU),
    (B, BIN + ["--pop-bubbles", "32"], 2, "--pop-bubbles MAXDIFF is at most 31\n"),
    (B, BIN + ["--correct", "0"], 2, "--correct N needs N >= 1 (or auto)\n"),
    (B, BIN + ["--max-insert", "0"], 2, "--max-insert N is 1..65535\n"),
    (B, ["--fastq", "r.fq", "31", "--world", "2"], 2, BUILDER_FASTQ_USAGE),
    (B, ["--fastq", "r.fq", "31", "--split", "0"], 2, BUILDER_FASTQ_USAGE),
    (B, BIN + ["--rounds", "5", "--rounds", "auto", "--walk-pairs", "2", "3"], 2, "unknown argument --walk-pairs\n"),
    (S, GKG, 2, "--cutoff C is required\n"),
    (S, GKG + ["--cutoff", "2", "--no-pairs"], 2, NO_PAIRS),
    (S, GKG + ["--cutoff", "2", "--no-pairs", "--thread-reads", "--range", "auto"], 2, NO_PAIRS),
    (S, GKG + ["--cutoff", "2", "--insert-hist", "x"], 2, MAX_INSERT),
    (S, GKG + ["--cutoff", "2", "--max-insert", "70000"], 2, MAX_INSERT),
    (S, ["g.gkg", "--fastq", "r.fq", "--cutoff", "2", "--world", "2"], 2, SIMPLIFIER_FASTQ_USAGE),
    (S, GKG + ["--cutoff", "2", "--range", "5"], 2, "unknown argument --range\n"),
    (C, BIN + ["--out", "o.bin", "--solid", "0"], 2, "usage: {exe} <reads.bin> <nreads> <k> --out <corrected.bin> [--solid N|auto] [--spectrum PATH]\n"),
    (K, ["g.gkg", "g.fa", "--bogus"], 2, "unknown argument --bogus\nusage: {exe} <graph.gkg> <genome.fasta> [--longer-than N] [--per-line] [--missing N]\n"),
    (V, ["a.fq", "o", "--bogus"], 2, "unknown argument --bogus\n"),
    (V, ["a.fq", "o", "--k", "0"], 2, "--split N needs N >= 1 and --k K needs 1 <= K <= 255\n"),
    # past every usage decision: the first thing a run does is open its reads (the options before it were all taken)
    (B, BIN + ["--walk-pairs", "2", "auto", "--clip-tips", "--pop-bubbles", "auto", "--contig-width", "0"], 1, "graph_builder: cannot open r.bin\n"),
    (S, GKG + ["--cutoff", "2", "--range", "auto", "--insert-hist", "h", "--thread-reads"], 1, "graph_simplifier: cannot open r.bin\n"),
]

# a value that is no number of the option's kind: one line that names the option, exit 2 (these aborted before)
MALFORMED = [
    (S, GKG + ["--cutoff", "abc"], "--cutoff"),
    (S, GKG + ["--cutoff", "2", "--take-first", "12x"], "--take-first"),
    (S, GKG + ["--cutoff", "2", "--contig-width", "-1"], "--contig-width"),
    (C, BIN + ["--out", "o.bin", "--solid", "x"], "--solid"),
    (B, ["r.bin", "31", "x"], "<k>"),
    (B, ["--fastq", "r.fq", "31", "--split", "x"], "--split"),
    (K, ["g.gkg", "g.fa", "--missing", "x"], "--missing"),
    (V, ["a.fq", "o", "--k", "1.5"], "--k"),
]


@pytest.fixture(scope="module")
def tools():
    if not all(os.path.exists(os.path.join(HOST, t)) for t in TOOLS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "genome_amd", "csrc"), "host"])
    return {t: os.path.join(HOST, t) for t in TOOLS}


def run(exe, args, cwd):
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=30, cwd=cwd)
    assert r.stdout == "" and os.listdir(cwd) == [], (r.stdout, os.listdir(cwd))
    return r


@pytest.mark.parametrize("tool", TOOLS)
def test_too_few_arguments_is_usage(tools, tmp_path, tool):
    for args in ([], ["x"]):
        r = run(tools[tool], args, tmp_path)
        assert r.returncode == 2 and r.stderr.startswith("usage: " + tools[tool] + " <") and r.stderr.count("\n") == 1, r.stderr


@pytest.mark.parametrize("tool,args,code,stderr", CASES, ids=[f"{c[0]}-{'_'.join(c[1][-3:])}" for c in CASES])
def test_usage_decision(tools, tmp_path, tool, args, code, stderr):
    r = run(tools[tool], args, tmp_path)
    assert (r.returncode, r.stderr) == (code, stderr.replace("{exe}", tools[tool]))


@pytest.mark.parametrize("tool,args,option", MALFORMED, ids=[f"{c[0]}-{c[2]}" for c in MALFORMED])
def test_malformed_number_names_the_option(tools, tmp_path, tool, args, option):
    r = run(tools[tool], args, tmp_path)
    assert r.returncode == 2 and r.stderr.startswith(option + " needs ") and r.stderr.count("\n") == 1 and args[-1] in r.stderr, r.stderr


def test_tool_common_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tool_common_check")
    # the runtimes linked in, as clang does by default: g++'s shared ASan runtime refuses to start where the environment preloads
    # any library ahead of it
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                            os.path.join(ROOT, "tests", "host", "tool_common_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0 and "warning" not in build.stderr, build.stderr[-4000:]
    env = dict(os.environ)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-4000:]
    assert "runtime error:" not in report and "AddressSanitizer" not in report and "LeakSanitizer" not in report, report[-4000:]
    assert "tool_common_check ok" in r.stdout
