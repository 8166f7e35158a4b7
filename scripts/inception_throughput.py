"""Throughput of the FID feature extractor (images/s, batch 50, 64 x 64 inputs, resize on): the conv_general.hip path
against the forced ``unfold`` lowering and against ``features_u8`` (a device uint8 tensor in, every pooling / the resize
/ the final average on csrc/fid_front.hip), interleaved in one process, warm-up, median of N batches each.

    python scripts/inception_throughput.py [--batches 24] [--out profiles/<name>.json]
    python scripts/inception_throughput.py --one-batch [--lowering unfold | u8]  # what rocprofv3 wraps: one timed batch
    python scripts/inception_throughput.py --merge-stats <kernel_stats.csv> --out <json> [--stats-key kernel_trace_u8]
        # total kernel time, launches per batch, the share outside the convolution kernel, ten most expensive kernels
    python scripts/inception_throughput.py --fid-epoch 1000 --out <json>   # one FID at n_samples by both routes
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


def merge_stats(path, out, key="kernel_trace"):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    top = [{"name": r["Name"][:160], "calls": int(float(r["Calls"])), "total_us": round(float(r["TotalDurationNs"]) / 1e3, 1),
            "share": round(float(r["TotalDurationNs"]) / total, 4)} for r in rows[:10]]
    rec = json.load(open(out)) if os.path.exists(out) else {}
    calls = sum(int(float(r["Calls"])) for r in rows)
    conv = sum(float(r["TotalDurationNs"]) for r in rows if "conv_general" in r["Name"])
    rec[key] = {"what": "rocprofv3 --kernel-trace --stats over --one-batch (warm-up batch + one batch: two batches, the first "
                        "with the one-time filter packs)",
                "total_kernel_us": round(total / 1e3, 1), "kernel_launches": calls, "launches_per_batch_incl_warmup": calls / 2,
                "conv_general_us": round(conv / 1e3, 1), "non_convolution_us": round((total - conv) / 1e3, 1), "top10": top}
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps({k: v for k, v in rec[key].items() if k != "top10"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=50)
    ap.add_argument("--one-batch", action="store_true")
    ap.add_argument("--lowering", default="hip")
    ap.add_argument("--merge-stats")
    ap.add_argument("--stats-key", default="kernel_trace")
    ap.add_argument("--fid-epoch", type=int, default=0, help="n_samples: time one FID by the file route and on the device")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.merge_stats:
        return merge_stats(a.merge_stats, a.out, a.stats_key)

    import torch
    from disentangle_mlp_amd import inception
    from oracle.inception import random_fid_inception
    ex = inception.InceptionFeatureExtractor(random_fid_inception(3).state_dict(), device="cuda", batch_size=a.batch_size)
    imgs = torch.randint(0, 256, (a.batch_size, 64, 64, 3), generator=torch.Generator().manual_seed(5)).float()

    imgs_u8 = imgs.to(torch.uint8).cuda()

    def batch(lowering):
        inception.CONV_LOWERING = "hip" if lowering == "u8" else lowering
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.features_u8(imgs_u8) if lowering == "u8" else ex(imgs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    if a.fid_epoch:
        return fid_epoch(a, ex)

    if a.one_batch:
        batch(a.lowering)
        print(json.dumps({"lowering": a.lowering, "seconds": batch(a.lowering)}))
        return
    for _ in range(a.warmup):
        batch("hip"), batch("unfold"), batch("u8")
    t = {"hip": [], "unfold": [], "u8": []}
    for _ in range(a.batches):
        for k in t:
            t[k].append(batch(k))

    def summary(v):
        ips = sorted(a.batch_size / s for s in v)
        return {"images_per_s_median": round(statistics.median(ips), 1), "images_per_s_min": round(ips[0], 1),
                "images_per_s_max": round(ips[-1], 1), "ms_per_batch_median": round(1e3 * statistics.median(v), 3)}

    rec = {"what": "InceptionFeatureExtractor, batch %d, 64x64 uint8 inputs, resize to 299 on; interleaved, %d warm-up + %d "
                   "timed batches per path, host clock around a synchronised batch" % (a.batch_size, a.warmup, a.batches),
           "device": torch.cuda.get_device_name(0), "kernel_path": summary(t["hip"]), "unfold_path": summary(t["unfold"]),
           "features_u8_path": summary(t["u8"])}
    rec["ratio_kernel_over_unfold"] = round(rec["kernel_path"]["images_per_s_median"] / rec["unfold_path"]["images_per_s_median"], 4)
    rec["ratio_features_u8_over_kernel"] = round(rec["features_u8_path"]["images_per_s_median"] / rec["kernel_path"]["images_per_s_median"], 4)
    print(json.dumps(rec))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        old.update(rec)
        json.dump(old, open(a.out, "w"), indent=1)


def fid_epoch(a, ex):
    """One epoch's FID at n_samples by both routes, once each (after one small warm-up of each): the file route writes
    PNGs (the reference's .pdf names are not found by get_fid's glob) and reads them back; the device route is
    fid.get_fid_of_generator.  Seeded decoder, reference statistics from the same network on seeded noise images."""
    import tempfile
    import torch
    from disentangle_mlp_amd import fid, image_io, model as M
    from disentangle_mlp_amd.trainer import ModelOpt
    torch.manual_seed(999)
    g = M.Generator_celeba(ModelOpt())
    g.apply(M.weights_init)
    g = g.cuda().train()
    n = a.fid_epoch
    with tempfile.TemporaryDirectory() as tmp:
        npz = os.path.join(tmp, "reference.npz")
        noise = torch.randint(0, 256, (100, 64, 64, 3), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
        st = fid.ActivationStatistics(2048, "cuda").update(ex.features_u8(noise))
        fid.save_statistics(npz, *st.finalize())

        def file_route(count, sub):
            d = os.path.join(tmp, sub)
            os.makedirs(d)
            with torch.no_grad():
                sample = g(torch.randn(count, 128).cuda())
                for i, x in enumerate(sample):
                    image_io.save_image(x, os.path.join(d, f"sample_{i}_0.png"), normalize=True)
            return fid.get_fid(d, npz, feature_extractor=ex)

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = f()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, v
        file_route(50, "warm"), fid.get_fid_of_generator(g, 50, 128, npz, feature_extractor=ex)
        t_file, v_file = timed(lambda: file_route(n, "timed"))
        t_dev, v_dev = timed(lambda: fid.get_fid_of_generator(g, n, 128, npz, feature_extractor=ex))
    rec = {"fid_epoch": {"what": "one FID at n_samples = %d, batch %d, once per route, host clock around a synchronised call; "
                                 "different latent draws per route" % (n, a.batch_size),
                         "file_route_png_seconds": round(t_file, 3), "on_device_seconds": round(t_dev, 3),
                         "fid_file_route": v_file, "fid_on_device": v_dev}}
    print(json.dumps(rec))
    if a.out:
        old = json.load(open(a.out)) if os.path.exists(a.out) else {}
        old.update(rec)
        json.dump(old, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
