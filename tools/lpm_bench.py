#!/usr/bin/env python3
"""Longest-prefix-match next hops (csrc/lpm.hip) over n = 2^24 destination
addresses, on the two route tables of nffacl.synth ("small": 100 routes, the
shape of examples/netlink.go; "large": about 500 000 routes, a BGP-like depth
mix).

  lds     LPM.lookup_device, the form that stages the top level in LDS
  global  LPM.lookup_device, the form that reads it from global memory
  torch   the same lookup as the reference writes it (packet.go:880-895), in
          torch over a DIR-24-8 this tool builds from the same routes:
          tbl24[addr >> 8], the ext mask, the tbl8 gather, the select, the hit
          test, the next hop — several passes of 4 n bytes each and one
          scattered gather into the 64 MB tbl24: the bar
  copy    a device-to-device copy of 8 n bytes (what one pass must move): the floor

Each round times K back-to-back launches between one HIP event pair, the
contenders alternating in this process; the JSON line holds every round's time
per launch, the medians and spreads (max - min over the rounds), lds / torch
with the bar's verdict and lds / copy (no bar), per table.  The first lookup of
every form is compared with the torch form over the whole batch.

--sweep also times both forms at n = 2^10 .. 2^24 on both tables (the crossover
behind the library's default choice of form).

usage: python tools/lpm_bench.py [--log2n 24] [--k 20] [--rounds 7] [--sweep] [--out profiles/lpm/lpm_bench.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "nff-go_amd"), str(ROOT / "tools")]
import nffacl  # noqa: E402
from nffacl import synth  # noqa: E402
from keys_encap_bench import summary, timed  # noqa: E402

HIT, EXT = 1 << 24, 1 << 25  # (torch has no uint32: the entry's flags sit above the 24-bit value)


def dir24_8(routes):
    """tbl24 (2^24 entries) and tbl8 (256 per group) of the routes as int32: value | HIT | EXT."""
    ip, depth, hop = routes
    tbl24, groups = np.zeros(1 << 24, np.int32), []
    for i in np.argsort(depth, kind="stable"):  # ascending depth: the longest prefix is written last
        d, a, leaf = int(depth[i]), int(ip[i]), int(hop[i]) | HIT
        if d <= 24:
            tbl24[a >> 8:(a >> 8) + (1 << (24 - d))] = leaf
            continue
        e = int(tbl24[a >> 8])
        if not e & EXT:
            groups.append(np.full(256, e, np.int32))
            e = tbl24[a >> 8] = (len(groups) - 1) | EXT
        groups[e & 0xFFFFFF][a & 0xFF:(a & 0xFF) + (1 << (32 - d))] = leaf
    return tbl24, np.concatenate(groups) if groups else np.zeros(256, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24, help="at least 6")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lpm" / "lpm_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lpm_bench.py needs a HIP device")
    n = 1 << a.log2n
    res = {"n": n, "k": a.k, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "tables": {}}
    for kind in ("small", "large"):
        routes = synth.gen_lpm_routes(kind)
        print(f"{kind}: {len(routes[0])} routes, {n} addresses", file=sys.stderr, flush=True)
        lpm = nffacl.CreateLPM(kind, 0, 1 << 20, 1 << 16)
        for ip, d, h in zip(*(x.tolist() for x in routes)):
            assert lpm.Add(ip, d, h) == 0
        lpm.commit()
        h24, h8 = dir24_8(routes)
        tbl24, tbl8 = torch.from_numpy(h24).cuda(), torch.from_numpy(h8).cuda()
        addr = torch.from_numpy(synth.gen_lpm_addresses(routes, n).view(np.int32)).cuda()
        nxt = torch.zeros(n, dtype=torch.int32, device="cuda")
        bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
        src, dst = (torch.zeros(2 * n, dtype=torch.int32, device="cuda") for _ in range(2))

        def in_torch(m=n):
            x = addr[:m]
            e = tbl24[(x >> 8) & 0xFFFFFF]
            ext = (e & EXT) != 0
            e = torch.where(ext, tbl8[((e & 0xFFFFFF) << 8 | (x & 0xFF)) * ext], e)
            hit = (e & HIT) != 0
            return torch.where(hit, e & 0xFFFFFF, 0), hit

        def form(flag, m=n):
            return lambda: lpm.lookup_device(addr, m, nxt, bits, flags=flag)

        contenders = {"lds": form(nffacl.LPM_FORCE_LDS), "global": form(nffacl.LPM_FORCE_GLOBAL),
                      "torch": in_torch, "copy": lambda: dst.copy_(src)}
        want, hit = in_torch()
        for name in ("lds", "global"):  # the same answers, or the numbers are void
            nxt.zero_(), bits.zero_()
            contenders[name]()
            torch.cuda.synchronize()
            assert torch.equal(nxt, want), f"{kind} {name}: next hops differ from the DIR-24-8 walk"
            packed = (hit.view(-1, 64).long() << torch.arange(64, device="cuda")).sum(1)  # (distinct bits: the OR)
            assert torch.equal(bits, packed), f"{kind} {name}: hit bits differ"
        for fn in contenders.values():  # warm-up: code objects, clocks
            timed(fn, 3)
        times = {name: [] for name in contenders}
        for _ in range(a.rounds):
            for name, fn in contenders.items():
                times[name].append(timed(fn, a.k))
        r = {"routes": len(routes[0]), "table_bytes": 4 * len(lpm.compile()), "dir24_8_bytes": 4 * (len(h24) + len(h8)),
             "hit_fraction": float(hit.float().mean()), **{name: summary(xs) for name, xs in times.items()}}
        r["lds_over_torch"] = r["lds"]["median_ms"] / r["torch"]["median_ms"]
        r["lds_no_slower_than_torch"] = r["lds"]["median_ms"] <= r["torch"]["median_ms"]
        r["lds_over_copy"] = r["lds"]["median_ms"] / r["copy"]["median_ms"]
        r["global_over_lds"] = r["global"]["median_ms"] / r["lds"]["median_ms"]
        if a.sweep:
            r["sweep_median_ms"] = {}
            for lg in range(10, a.log2n + 1, 2):
                k = max(a.k, min(200, (1 << 26) >> lg))
                pair = {name: form(flag, 1 << lg) for name, flag in (("lds", nffacl.LPM_FORCE_LDS),
                                                                      ("global", nffacl.LPM_FORCE_GLOBAL))}
                xs = {name: [] for name in pair}
                for _ in range(a.rounds):
                    for name, fn in pair.items():
                        xs[name].append(timed(fn, k))
                r["sweep_median_ms"][str(lg)] = {name: summary(v)["median_ms"] for name, v in xs.items()}
        res["tables"][kind] = r
        torch.cuda.synchronize()
        lpm.Free()
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
