"""Throughput of the FID feature extractor (images/s, batch 50, 64 x 64 inputs, resize on): the conv_general.hip path
against the forced ``unfold`` lowering, interleaved in one process, warm-up, median of N batches each.

    python scripts/inception_throughput.py [--batches 24] [--out profiles/<name>.json]
    python scripts/inception_throughput.py --one-batch [--lowering unfold]     # what rocprofv3 wraps: one timed batch
    python scripts/inception_throughput.py --merge-stats <kernel_stats.csv> --out <json>   # ten most expensive kernels
Seeded random weights (oracle.inception.random_fid_inception): the pretrained file cannot be obtained offline."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def merge_stats(path, out):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    top = [{"name": r["Name"][:160], "calls": int(float(r["Calls"])), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
            "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows[:10]]
    rec = json.load(open(out)) if os.path.exists(out) else {}
    rec["kernel_trace"] = {"what": "rocprofv3 --kernel-trace --stats over --one-batch (warm-up batch + one batch, kernel path)",
                           "total_kernel_us": round(total / 1e3, 1), "top10": top}
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec["kernel_trace"]["top10"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--one-batch", action="store_true")
    ap.add_argument("--lowering", default="hip")
    ap.add_argument("--merge-stats")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out)

    import torch
    from disentangle_mlp_amd import inception
    from oracle.inception import random_fid_inception
    ex = inception.InceptionFeatureExtractor(random_fid_inception(3).state_dict(), device="cuda", batch_size=a.batch_size)
    imgs = torch.randint(0, 256, (a.batch_size, 64, 64, 3), generator=torch.Generator().manual_seed(5)).float()

    def batch(lowering):
        inception.CONV_LOWERING = lowering
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex(imgs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if a.one_batch:
        batch(a.lowering)
        print(json.dumps({"lowering": a.lowering, "seconds": batch(a.lowering)}))
        return
    for _ in range(a.warmup):
        batch("hip"), batch("unfold")
    t = {"hip": [], "unfold": []}
    for _ in range(a.batches):
        for k in t:
            t[k].append(batch(k))

    def summary(v):
        ips = sorted(a.batch_size / s for s in v)
        return {"images_per_s_median": round(statistics.median(ips), 1), "images_per_s_min": round(ips[0], 1),
                "images_per_s_max": round(ips[-1], 1), "ms_per_batch_median": round(1e3 * statistics.median(v), 3)}

    rec = {"what": "InceptionFeatureExtractor, batch %d, 64x64 uint8 inputs, resize to 299 on; interleaved, %d warm-up + %d "
                   "timed batches per path, host clock around a synchronised batch" % (a.batch_size, a.warmup, a.batches),
           "device": torch.cuda.get_device_name(0), "kernel_path": summary(t["hip"]), "unfold_path": summary(t["unfold"])}
    rec["ratio_kernel_over_unfold"] = round(rec["kernel_path"]["images_per_s_median"] / rec["unfold_path"]["images_per_s_median"], 4)
    print(json.dumps(rec))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        old.update(rec)
        json.dump(old, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
