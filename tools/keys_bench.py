#!/usr/bin/env python3
"""Key path (nffacl_key, csrc/keys.hip) against the slot path on the same
packets and rules, in one process, at n = 2^24, for the C2 and C5 rule sets:

  kernel      classify_device (64-byte slots) vs classify_keys_device on the
              keys extract_keys_device made of those slots — K back-to-back
              launches between one HIP event pair per round, the two
              contenders alternating, verdicts compared once (exact)
  extract     extract_keys_device alone, the same way
  host        classify_host vs classify_keys_host on pinned arrays (the kernel
              reads them over the link), host clock around the synchronous call

The JSON line holds every round's time per launch, medians, spreads (max - min
over the rounds), the ratios and the bytes per packet each path moves.

usage: python tools/keys_bench.py [--log2n 24] [--k 50] [--rounds 7] [--host-reps 5]
                                  [--out profiles/keys/keys_bench.json]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
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


def wall(fn, reps):
    """ms per synchronous call, host clock."""
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def summary(xs):
    return {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "rounds_ms": xs}


def case(name, n, k, rounds, host_reps):
    print(f"{name}: {n} packets", file=sys.stderr, flush=True)
    g = synth.gen_rules(synth.SPECS[name], synth.RULE_SEEDS[name])
    h_slots = torch.from_numpy(synth.gen_slots(g, n, synth.PACKET_SEEDS[name])).pin_memory()
    slots = h_slots.to("cuda")
    keys = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    key6 = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    p_slots = torch.zeros(n, dtype=torch.int32, device="cuda")
    p_keys = torch.zeros(n, dtype=torch.int32, device="cuda")
    with nffacl.Engine(nffacl.L3Rules.parse_text(g.text)) as eng:
        ki = eng.kernel_info()

        def by_slots():
            eng.classify_device(slots, 64, n, p_slots)

        def by_keys():
            eng.classify_keys_device(keys, key6, n, n, p_keys)

        def extract():
            nffacl.extract_keys_device(slots, 64, n, keys, key6)

        for fn in (extract, by_slots, by_keys):  # warm-up: code objects, LDS attributes
            timed(fn, 3)
        exact = bool(torch.equal(p_slots, p_keys))
        t_slots, t_keys = [], []
        for _ in range(rounds):
            t_slots.append(timed(by_slots, k))
            t_keys.append(timed(by_keys, k))
        t_extract = [timed(extract, k) for _ in range(rounds)]
        torch.cuda.synchronize()
        n6 = int(((keys[:, 3] >> 8) == 6).sum())
        # host-inclusive: pinned inputs and outputs, read and written over the link
        h_keys = keys.cpu().pin_memory()
        h_key6 = key6.cpu().pin_memory()
        h_port = torch.zeros(n, dtype=torch.int32).pin_memory()
        out = h_port.numpy().view(np.uint32)
        nk = h_keys.numpy().view(nffacl.KEY_DTYPE).reshape(-1)
        nk6 = h_key6.numpy().view(nffacl.KEY6_DTYPE).reshape(-1)
        ns = h_slots.numpy()

        def host_slots():
            eng.classify_host(ns, 64, n, out=out, permit=False)

        def host_keys():
            eng.classify_keys_host(nk, nk6, n, out=out, permit=False)

        host_slots()
        want = out.copy()
        host_keys()
        host_exact = bool((out == want).all()) and bool((want == p_slots.cpu().numpy().view(np.uint32)).all())
        w_slots, w_keys = [], []
        for _ in range(host_reps):
            w_slots += wall(host_slots, 1)
            w_keys += wall(host_keys, 1)
    s, q, e = summary(t_slots), summary(t_keys), summary(t_extract)
    hs, hk = summary(w_slots), summary(w_keys)
    return {"case": name, "walk": ki.walk, "slots": ki.slots, "block": ki.block, "per_cu": ki.per_cu,
            "ipv6_fraction": n6 / n, "exact_keys_vs_slots": exact, "host_exact": host_exact,
            "kernel_slots": s, "kernel_keys": q, "extract": e,
            "keys_over_slots": q["median_ms"] / s["median_ms"],
            "keys_faster_beyond_spread": min(t_slots) - max(t_keys) > 0,
            "bytes_per_packet": {"slots": 68, "keys": 20 + 32 * n6 / n, "extract": 64 + 16 + 32 * n6 / n},
            "gpps": {"slots": n / s["median_ms"] / 1e6, "keys": n / q["median_ms"] / 1e6,
                     "extract": n / e["median_ms"] / 1e6},
            "host_slots": hs, "host_keys": hk,
            "host_gpps": {"slots": n / hs["median_ms"] / 1e6, "keys": n / hk["median_ms"] / 1e6},
            "host_keys_over_slots": hk["median_ms"] / hs["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keys" / "keys_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keys_bench.py needs a HIP device")
    n = 1 << a.log2n
    res = {"n": n, "k": a.k, "rounds": a.rounds, "host_reps": a.host_reps,
           "device": torch.cuda.get_device_name(0),
           "cases": [case(c, n, a.k, a.rounds, a.host_reps) for c in ("c2", "c5")]}
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
