"""Developer tool: the autoregressive sampler of a PixelVAE two ways, in one process on one GPU -- main.generate's default path (the
reference's Python loop: S * S times cat + run_pixelcnn + softmax + multinomial + indexed write) against VAE.sample_pixels (the whole
loop enqueued by one C call).  PixelVAE with S = 64, 4 PixelCNN layers, 32 intermediate channels, Q = 2.  Per cell (dtype, N): one warm-up
call, then `--repeats` timed calls, wall time around a final synchronise; min and mean in seconds.  Also times the host side of
sample_pixels alone (the call returns when everything is enqueued).  In each cell sample_pixels is timed before the loop, each after a
warm-up call of its own.
usage: python tools/sampler_bench.py [--n 16 128] [--dtypes bf16 f32] [--repeats 3] [--size 64] [--json FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
M = importlib.import_module("moving-mnist-vae_amd.model")
main = importlib.import_module("moving-mnist-vae_amd.main")
MEAN, STD = 0.0521, 0.2222


def timed(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def run(args):
    dev = torch.device("cuda")
    S, rows = args.size, []
    for dt in args.dtypes:
        torch.manual_seed(0)
        m = M.VAE(1, 32, 2, 2, 32, True, False, 4, "ReLu", 1, 1, 0, True, 0.0, S, compute_dtype=dt).to(dev).eval()
        for N in args.n:
            with torch.no_grad():
                z_image = m.get_z_image(torch.randn(N, 32, 1, 1, device=dev)).float()
            u = torch.rand(N, S * S, device=dev)
            enqueue = []

            def loop():
                main.generate(z_image, torch.zeros(N, 1, S, S, device=dev), m, MEAN, STD)

            def device():
                t0 = time.perf_counter()
                m.sample_pixels(torch.zeros(N, 1, S, S, device=dev), z_image, data_mean=MEAN, data_std=STD, uniforms=u)
                enqueue.append(time.perf_counter() - t0)

            row = {"dtype": dt, "N": N, "S": S}
            for name, fn in (("sample_pixels", device), ("generate_loop", loop)):
                fn()                                          # warm-up
                del enqueue[:]
                ts = timed(fn, args.repeats)
                row[name] = {"min_s": min(ts), "mean_s": sum(ts) / len(ts), "all_s": ts}
                if name == "sample_pixels":
                    row[name]["enqueue_mean_s"] = sum(enqueue) / len(enqueue)
            row["faster"] = row["sample_pixels"]["mean_s"] < row["generate_loop"]["min_s"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.json:
                with open(args.json, "w") as f:
                    json.dump(rows, f, indent=1)
    print(f"{'dtype':6}{'N':>5}  {'loop min':>10}{'loop mean':>11}  {'device min':>11}{'device mean':>12}{'enqueue':>9}  mean < loop min")
    for r in rows:
        l, d = r["generate_loop"], r["sample_pixels"]
        print(f"{r['dtype']:6}{r['N']:>5}  {l['min_s']:>10.3f}{l['mean_s']:>11.3f}  {d['min_s']:>11.3f}{d['mean_s']:>12.3f}{d['enqueue_mean_s']:>9.3f}  {r['faster']}")
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "f32"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--json", default=None)
    run(ap.parse_args())
