#!/usr/bin/env python3
"""Packed-frame gather and frame keys (csrc/route_frames.hip, keys.hip) on C3's
IMIX batch at n = 2^24 frames, routed by its own verdicts (ROUTE_SEPARATE):

  gather   Router.gather_frames over the route's whole index, against a
           hipMemcpyAsync device-to-device copy of the same out_bytes — the
           ceiling for reading and writing that many bytes once
  keys     extract_keys_frames_device against extract_keys_device on 64-byte
           slots holding the same headers

Each round times K back-to-back launches between one HIP event pair, the two
contenders alternating in this process; the JSON line holds every round's time
per launch, the medians, the spread (max - min over the rounds) and the
gather/copy and frames/slots ratios.  The gathered batch is checked once: its
descriptors' lengths and its first 16-byte chunks against the source's.
(`keys_equal_slots_keys` is recorded, not required: a slot holds a frame's
first 64 bytes, so ports that IP options push past byte 63 differ.)

usage: python tools/route_frames_bench.py [--log2n 24] [--k 20] [--rounds 7] [--align 64]
                                          [--out profiles/route_frames/route_frames_bench.json]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "nff-go_amd")]
import nffacl  # noqa: E402
from nffacl import synth  # noqa: E402


def timed(fn, k):
    """ms per call of k back-to-back calls between one event pair."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def summary(xs):
    return {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "rounds_ms": xs}


def alternate(f, g, k, rounds):
    for fn in (f, g):
        timed(fn, 3)  # warm-up: code objects, clocks
    tf, tg = [], []
    for _ in range(rounds):
        tf.append(timed(f, k))
        tg.append(timed(g, k))
    return summary(tf), summary(tg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--align", type=int, default=64)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "route_frames" / "route_frames_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("route_frames_bench.py needs a HIP device")
    n = 1 << a.log2n
    g = synth.gen_rules(synth.SPECS["c3"], synth.RULE_SEEDS["c3"])
    print(f"c3 imix: {n} frames", file=sys.stderr, flush=True)
    h_frames, h_desc = synth.gen_imix(g, n, synth.PACKET_SEEDS["c3"])
    frames, desc = torch.from_numpy(h_frames).to("cuda"), torch.from_numpy(h_desc.view("int64")).to("cuda")
    del h_frames
    port, index = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    offsets = torch.zeros(4, dtype=torch.int32, device="cuda")
    out, copy = torch.empty_like(frames), torch.empty_like(frames)
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    cap = frames.numel() // 16 * 16
    with nffacl.Engine(nffacl.L3Rules.parse_text(g.text)) as eng, nffacl.Router(nffacl.ROUTE_SEPARATE, 2, n) as router:
        eng.classify_frames_device(frames, desc, n, port)
        router.route(port, n, index, offsets)

        def gather():
            router.gather_frames(frames, desc, n, index, n, out, cap, out_desc, out_bytes, a.align)

        gather()
        torch.cuda.synchronize()
        nbytes = int(out_bytes.cpu()[0])
        assert nbytes <= cap, (nbytes, cap)
        src = desc[index.long()]
        same_len = bool(torch.equal(out_desc & 0xFFFF, src & 0xFFFF))
        same_head = bool(torch.equal(out.view(-1, 16)[out_desc >> 20], frames.view(-1, 16)[src >> 20]))
        del src

        def memcpy():
            copy[:nbytes].copy_(frames[:nbytes], non_blocking=True)

        t_gather, t_copy = alternate(gather, memcpy, a.k, a.rounds)
        del out, copy
        # keys: the frames against 64-byte slots of the same first lines (IMIX rooms are 64-byte aligned)
        slots = frames.view(-1, 64)[desc >> 22].contiguous()
        keys, key6 = torch.zeros((n, 4), dtype=torch.int32, device="cuda"), torch.zeros((n, 8), dtype=torch.int32, device="cuda")
        keys_s = torch.zeros_like(keys)
        t_kf, t_ks = alternate(lambda: nffacl.extract_keys_frames_device(frames, desc, n, keys, key6),
                               lambda: nffacl.extract_keys_device(slots, 64, n, keys_s, key6), a.k, a.rounds)
        same_keys = bool(torch.equal(keys, keys_s))
        torch.cuda.synchronize()
    res = {"n": n, "k": a.k, "rounds": a.rounds, "align": a.align, "device": torch.cuda.get_device_name(0),
           "out_bytes": nbytes, "segment_sizes": offsets.cpu().tolist(), "lengths_equal": same_len,
           "first_chunks_equal": same_head, "keys_equal_slots_keys": same_keys,
           "gather": t_gather, "memcpy_d2d": t_copy, "gather_over_copy": t_gather["median_ms"] / t_copy["median_ms"],
           "gather_gbps_read_plus_write": 2 * nbytes / t_gather["median_ms"] / 1e6,
           "keys_frames": t_kf, "keys_slots": t_ks, "frames_over_slots": t_kf["median_ms"] / t_ks["median_ms"]}
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
