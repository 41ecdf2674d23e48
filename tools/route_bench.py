#!/usr/bin/env python3
"""Routing stage (nffacl.Router, csrc/route.hip) against what a user runs today
for the same lists, torch.sort(port, stable=True), at n = 2^24 on two verdict
vectors made by the classify kernels in this process:

  c2_separate   the C2 rule set's verdicts, ROUTE_SEPARATE (n_out = 2)
  fwd_split5    forwarding.conf's verdicts (outputs 0..4), ROUTE_SPLIT, n_out = 5

Each round times K back-to-back launches between one HIP event pair, the two
contenders alternating; the JSON line holds every round's time per launch,
the medians, the spread (max - min over the rounds) and the classify kernel's
time on the same packets.  The route result is checked once against the
sort's indices (exact).

usage: python tools/route_bench.py [--log2n 24] [--k 100] [--rounds 7] [--out profiles/route/route_bench.json]"""
import argparse
import json
import statistics
import sys
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


def summary(xs):
    return {"median_ms": statistics.median(xs), "spread_ms": max(xs) - min(xs), "rounds_ms": xs}


def case(name, text, gen, seed, mode, n_out, n, k, rounds):
    print(f"{name}: {n} packets", file=sys.stderr, flush=True)
    slots = torch.from_numpy(synth.gen_slots(gen, n, seed)).to("cuda")
    port = torch.zeros(n, dtype=torch.int32, device="cuda")
    index = torch.zeros(n, dtype=torch.int32, device="cuda")
    offsets = torch.zeros(n_out + 2, dtype=torch.int32, device="cuda")
    with nffacl.Engine(nffacl.L3Rules.parse_text(text)) as eng, nffacl.Router(mode, n_out, n) as router:
        def classify():
            eng.classify_device(slots, 64, n, port)

        def route():
            router.route(port, n, index, offsets)

        def sort():
            return torch.sort(port, stable=True)

        for fn in (classify, route, sort):  # warm-up: code objects, the sort's workspace
            timed(fn, 3)
        key = (port != 0).to(torch.int32) if mode == nffacl.ROUTE_SEPARATE else port
        exact = bool(torch.equal(index, torch.sort(key, stable=True).indices.to(torch.int32)))
        t_route, t_sort = [], []
        for _ in range(rounds):
            t_route.append(timed(route, k))
            t_sort.append(timed(sort, k))
        t_classify = [timed(classify, k) for _ in range(rounds)]
        torch.cuda.synchronize()
        counts = np.diff(offsets.cpu().numpy().astype(np.int64)).tolist()
    r, s, c = summary(t_route), summary(t_sort), summary(t_classify)
    return {"case": name, "n_out": n_out, "segment_sizes": counts, "exact_vs_sort": exact,
            "route": r, "torch_stable_sort": s, "classify": c,
            "sort_over_route": s["median_ms"] / r["median_ms"],
            "faster_beyond_spread": min(t_sort) - max(t_route) > 0,
            "route_share_of_classify": r["median_ms"] / c["median_ms"],
            "route_gbps_at_12B_per_packet": 12 * n / r["median_ms"] / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "route" / "route_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("route_bench.py needs a HIP device")
    n = 1 << a.log2n
    c2 = synth.gen_rules(synth.SPECS["c2"], synth.RULE_SEEDS["c2"])
    fwd = (ROOT / "tests" / "golden" / "rules" / "forwarding.conf").read_text()
    res = {"n": n, "k": a.k, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "cases": [
        case("c2_separate", c2.text, c2, synth.PACKET_SEEDS["c2"], nffacl.ROUTE_SEPARATE, 2, n, a.k, a.rounds),
        case("fwd_split5", fwd, synth.firewall_rules(fwd), 11, nffacl.ROUTE_SPLIT, 5, n, a.k, a.rounds)]}
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
