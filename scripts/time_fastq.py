"""Time FASTQ -> `.bin` on the device (gk_fastq_convert / gk_fastq_count) at C2's shape: 10^6 pairs of 2 x 150 bases, N injected,
qualities attached (~0.65 GB of text).  Prints one JSON object (and writes it to --out):

  convert      gk_fastq_convert from pinned host text to a pinned host `.bin`: ms and GB/s of text, gk_fastq_last_ms's split
  upload       the same bytes through gk_dev_upload alone
  count        gk_fastq_count (k = 31) against gk_fastq_convert + gk_map_count_reads of the converted stream
  python       the plain restatement tests/fastq_ref.py on a 10^4-pair sample, for scale only

Run the parse kernels under `rocprofv3 --kernel-trace --stats -- python scripts/time_fastq.py --reps 1` for their device time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from genome_amd.dnamap import Context, HipDNAMap  # noqa: E402
from genome_amd.fastq import FastqReader  # noqa: E402


def synth_fastq(ctx, npairs: int, mate_len: int = 150, n_rate: float = 0.001) -> np.ndarray:
    """records of gk_synth_reads_dev (mode G) as FASTQ: one sequence line = mate 1 ++ mate 2, quality line of equal length"""
    stride = 1 + (mate_len + 3) // 4
    d = ctx.alloc(2 * npairs * stride + 64)
    ctx.synth_reads(d, 2 * npairs, mate_len, "G", 2, 0, 5_000_000, 0.01)
    rec = ctx.download(d, 2 * npairs * stride).reshape(2 * npairs, stride)[:, 1:]
    ctx.free(d)
    codes = np.stack([(rec >> (2 * j)) & 3 for j in range(4)], axis=2).reshape(2 * npairs, -1)[:, :mate_len]
    seq = np.frombuffer(b"AGCT", np.uint8)[codes].reshape(npairs, 2 * mate_len)
    rng = np.random.default_rng(7)
    seq[rng.random(seq.shape) < n_rate] = ord("N")
    hdr = b"@synthetic\n"
    L2 = 2 * mate_len
    a = np.empty((npairs, len(hdr) + L2 + 3 + L2 + 1), np.uint8)
    a[:, :len(hdr)] = np.frombuffer(hdr, np.uint8)
    o = len(hdr)
    a[:, o:o + L2] = seq
    a[:, o + L2:o + L2 + 3] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, o + L2 + 3:o + 2 * L2 + 3] = rng.integers(ord("!"), ord("J"), (npairs, L2), dtype=np.uint8)
    a[:, -1] = ord("\n")
    return a.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = Context(0)
    text = synth_fastq(ctx, args.pairs)
    n = text.size
    pinned = ctx.host_alloc(n)
    pinned[:] = text
    bin_out = ctx.host_alloc(n)
    res = {"pairs": args.pairs, "text_bytes": n, "split_at": 150}

    def convert_once():
        rd = FastqReader(ctx, 150, 23)
        import ctypes as C
        from genome_amd import _lib as L
        nb = C.c_size_t()
        t0 = time.perf_counter()
        L.check(L.lib().gk_fastq_convert(rd.h, pinned.ctypes.data, n, 1, bin_out.ctypes.data, n, C.byref(nb)), ctx.h)
        ms = (time.perf_counter() - t0) * 1e3
        split = rd.last_ms()
        st = rd.stats()
        rd.close()
        return ms, split, st, nb.value

    conv = [convert_once() for _ in range(args.reps + 1)][1:]
    best = min(conv, key=lambda x: x[0])
    res["convert"] = {"ms": [round(c[0], 3) for c in conv], "best_ms": round(best[0], 3), "GBps_text": round(n / best[0] / 1e6, 2),
                      "last_ms": {k: round(v, 3) for k, v in best[1].items()}, "stats": best[2], "bin_bytes": best[3]}
    d = ctx.alloc(n)
    up = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        ctx.upload(d, pinned)
        up.append((time.perf_counter() - t0) * 1e3)
    ctx.free(d)
    up = up[1:]
    res["upload"] = {"ms": [round(x, 3) for x in up], "best_ms": round(min(up), 3), "GBps": round(n / min(up) / 1e6, 2)}
    res["convert_over_upload"] = round(best[0] / min(up), 3)
    res["parse_kernels_over_upload"] = round(best[1]["kernels"] / min(up), 3)

    k = 31
    bin_bytes = bin_out[:best[3]].copy()
    cnt, two = [], []
    for _ in range(args.reps):
        m = HipDNAMap(ctx, k, 0)
        rd = FastqReader(ctx, 150, 23)
        t0 = time.perf_counter()
        occ = rd.count(m, pinned, last=True)
        cnt.append((time.perf_counter() - t0) * 1e3)
        split = rd.last_ms()
        ver = m.verify_checksum()
        rd.close(); m.close()
        m = HipDNAMap(ctx, k, 0)
        t0 = time.perf_counter()
        rd = FastqReader(ctx, 150, 23)
        nb = len(rd.convert(pinned, last=True))
        occ2 = m.count_reads(bin_out[:nb], 2 * args.pairs)
        two.append((time.perf_counter() - t0) * 1e3)
        assert occ == occ2 and m.verify_checksum() == ver
        rd.close(); m.close()
    res["count_k31"] = {"fastq_count_ms": [round(x, 3) for x in cnt], "convert_then_count_reads_ms": [round(x, 3) for x in two],
                        "occurrences": occ, "last_ms": {k_: round(v, 3) for k_, v in split.items()}, "tables_equal": True}
    del bin_bytes

    import fastq_ref
    sample = text[:10_000 * (text.size // args.pairs)].tobytes()
    t0 = time.perf_counter()
    fastq_ref.convert(sample, 150, 23)
    res["python_restatement_1e4_pairs_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    ctx.host_free(pinned); ctx.host_free(bin_out)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
