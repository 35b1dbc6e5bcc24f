#!/usr/bin/env python3
"""time range_search on the three workloads of the flat index, device in / device out and numpy in / numpy out, against search(k=10)
on the same inputs:
    C1           1,000,000 x 768 Gaussian bf16 rows, 65,536 queries, inner product (the bf16 form of the scan)
    fingerprint  500,000 x 2048 signed integer counts (retrieve_faiss.py:24-27 class), 65,536 queries, L2 (the int8 form)
    morgan       500,000 x 1024 bit vectors (retrieve_faiss.py:36-44 class), 65,536 queries, L2 (the fp4 form)
Radii for about 10, 100 and 1,000 results per query are the median k-th distance of a search(k) over 1,024 of the queries.
    python tools/range_probe.py [--workloads c1,fingerprint,morgan] [--reps 3] [--out range_probe.jsonl]
(under rocprofv3 --kernel-trace --stats for the per-kernel table)"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import textreact_amd.faiss_compat as faiss


def workload(name, g):
    nq = 65_536
    if name == "c1":
        y = torch.randn((1_000_000, 768), generator=g, device="cuda").bfloat16()
        x = torch.randn((nq, 768), generator=g, device="cuda").bfloat16()
        return faiss.IndexFlatIP(768), y, x
    if name == "fingerprint":      # ~2 % of the components nonzero, counts in [-10, 10]
        def fp(n):
            v = torch.randint(-10, 11, (n, 2048), generator=g, device="cuda").float()
            return (v * (torch.rand((n, 2048), generator=g, device="cuda") < 0.02)).bfloat16()
        return faiss.IndexFlatL2(2048), fp(500_000), fp(nq)
    def bits(n):                   # Morgan-like: 5 % of the bits set
        return (torch.rand((n, 1024), generator=g, device="cuda") < 0.05).bfloat16()
    return faiss.IndexFlatL2(1024), bits(500_000), bits(nq)


def timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(); t1 = time.perf_counter()
        best = (t1 - t0) * 1e3 if best is None else min(best, (t1 - t0) * 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c1,fingerprint,morgan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--targets", default="10,100,1000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    lines = []
    for name in a.workloads.split(","):
        idx, y, x = workload(name, g)
        idx.add(y)
        idx.set_timing(True)
        ms_k10, _ = timed(lambda: idx.search(x, 10), a.reps)
        st = idx.last_stats()
        base = {"workload": name, "n": y.shape[0], "d": y.shape[1], "nq": x.shape[0],
                "metric": "IP" if isinstance(idx, faiss.IndexFlatIP) else "L2"}
        rec = dict(base, call="search_k10_device", ms=round(ms_k10, 2), scan_ms=round(st["scan_ms"], 2), int8_scan=st["int8_scan"])
        print(json.dumps(rec), flush=True); lines.append(rec)
        xh = x.float().cpu().numpy()
        for t in (int(v) for v in a.targets.split(",")):
            Ds, _ = idx.search(x[:1024], t)
            r = float(Ds[:, -1].float().median())
            ms_dev, (lims, D, I) = timed(lambda: idx.range_search(x, r), a.reps)
            rs = idx.last_range_stats()
            ms_host, (lh, Dh, Ih) = timed(lambda: idx.range_search(xh, r), 1)
            same = bool(np.array_equal(lh, lims.cpu().numpy()) and np.array_equal(Ih, I.cpu().numpy())
                        and np.array_equal(Dh.view(np.uint32), D.cpu().numpy().view(np.uint32)))
            rec = dict(base, call="range_search", target=t, radius=r, results_per_query=round(rs["n_results"] / x.shape[0], 1),
                       ms_device=round(ms_dev, 2), scan_ms=round(rs["scan_ms"], 2), total_ms=round(rs["total_ms"], 2),
                       ms_host=round(ms_host, 2), n_exact=rs["n_exact"], n_splits=rs["n_splits"], int8_scan=rs["int8_scan"],
                       host_equals_device=same, vs_search_k10=round(ms_dev / ms_k10, 2))
            print(json.dumps(rec), flush=True); lines.append(rec)
        del idx, y, x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
