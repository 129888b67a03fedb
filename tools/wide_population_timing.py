#!/usr/bin/env python3
"""Device times of MultisampleVariantsDetector on a population of more than 255 samples (KPM
`k_posterior_wide`): a synthetic population on one contig through a staged run, `scan_ms` (KLM + KQN) and
`genotype_ms` (the mask kernel, stage A and KPM) of `stats()` over --steps passes after --warmup.

--oracle instead measures the CPU restatement on the same population model: one oracle process per core (at most
--procs) on its own --oracle-length contig, wall time over the pool (the way bench.py's CPU baseline runs it), and the
time one contig of --length would take at that rate.

Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools", "synth")):
    if p not in sys.path:
        sys.path.insert(0, p)


def synth(args, length, seed):
    import pysynth
    return pysynth.Synth(genome=pysynth.CUSTOM, custom_len=length, seed=seed, n_samples=args.samples, depth=args.depth,
                         snv_rate=args.snv_rate, quality_model=2)


def gpu(args):
    from ngsepcore_amd import GpuPileupSession, default_params
    t0 = time.time()
    syn = synth(args, args.length, args.seed)
    rgs = [(f"S{k:03d}", f"S{k:03d}") for k in range(args.samples)]
    p = default_params()
    p.multisample = 1
    scan, geno = [], []
    with GpuPileupSession(p) as s:
        s.set_samples(rgs)
        for name, seq in syn.contigs():
            s.set_reference(name, seq)
        s.stage(syn.batch())
        s.stage_finish()
        t_stage = time.time() - t0
        for k in range(args.warmup + args.steps):
            s.run_staged()
            st = s.stats()
            if k >= args.warmup:
                scan.append(st.scan_ms)
                geno.append(st.genotype_ms)
    scan.sort()
    geno.sort()
    return {"what": "gpu staged run", "samples": args.samples, "depth": args.depth, "length": args.length,
            "steps": args.steps, "scan_ms": {"min": scan[0], "median": scan[len(scan) // 2], "max": scan[-1]},
            "genotype_ms": {"min": geno[0], "median": geno[len(geno) // 2], "max": geno[-1]},
            "positions_genotyped": st.positions_genotyped, "hard_sites": st.hard_sites, "sites_called": st.sites_called,
            "generate_and_stage_s": round(t_stage, 1)}


def oracle(args):
    cli = os.path.join(ROOT, "oracle", "build", "ngsep_oracle")
    procs_n = min(args.procs, os.cpu_count() or 1)
    with tempfile.TemporaryDirectory() as d:
        pieces = []
        for k in range(procs_n):
            syn = synth(args, args.oracle_length, args.seed + 1000 * k)
            fa, sam, _ = syn.write(os.path.join(d, f"piece{k}"))
            syn.close()
            pieces.append((fa, sam))
        t0 = time.perf_counter()
        procs = [subprocess.Popen([cli, "MultisampleVariantsDetector", "-r", fa, "-o", os.path.join(d, f"o{k}.vcf"), sam],
                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) for k, (fa, sam) in enumerate(pieces)]
        for pr in procs:
            if pr.wait() != 0:
                raise RuntimeError("oracle failed")
        wall = time.perf_counter() - t0
    rate = procs_n * args.oracle_length / wall
    return {"what": "oracle (CPU restatement)", "samples": args.samples, "depth": args.depth, "processes": procs_n,
            "piece_length": args.oracle_length, "wall_s": round(wall, 2), "positions_per_s": round(rate, 1),
            "seconds_for_length": round(args.length / rate, 1), "length": args.length}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--depth", type=float, default=4.0)
    ap.add_argument("--length", type=int, default=1_000_000)
    ap.add_argument("--snv-rate", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=52)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--oracle-length", type=int, default=4000)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    print(json.dumps(oracle(args) if args.oracle else gpu(args)))


if __name__ == "__main__":
    main()
