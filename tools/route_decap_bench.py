#!/usr/bin/env python3
"""Decapsulating packed-frame gather (csrc/route_decap.hip) on C3's IMIX batch
at n = 2^24 frames with every frame wrapped in 8-byte GTP-U over IPv4 (36
bytes of shims, the batch of tools/keys_encap_bench.py).  Cursors and keys
come from extract_keys_encap_frames_device; the batch is routed SEPARATE by
the verdicts of those keys.

  decap   Router.gather_decap_frames over the route's whole index
  plain   Router.gather_frames of the same index over the same batch: the
          yardstick; it reads the same bytes and writes the shims as well
  alt     (--alt-lib) decap of a second build of the library, e.g. an
          experiment build `make EXTRA=-D... OBJDIR=... OUT=...`

Checked before timing: extract_keys_frames_device on decap's output gives the
encap keys of the frames it gathered.  Each round times K back-to-back
launches between one HIP event pair, the contenders alternating in this
process; the JSON line holds every round's time per launch, the medians, the
spreads (max - min over the rounds), the ratios to `plain`, the bytes each
call reads and writes, and whether decap's median is within plain's plus the
larger of the two spreads.

usage: python tools/route_decap_bench.py [--log2n 24] [--k 20] [--rounds 7] [--align 64] [--alt-lib LIB.so]
                                         [--out profiles/route_decap/route_decap_bench.json]"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "nff-go_amd"), str(ROOT / "tools")]
import nffacl  # noqa: E402
from nffacl import synth  # noqa: E402
from keys_encap_bench import summary, timed, wrap_gtpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--align", type=int, default=64)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "route_decap" / "route_decap_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("route_decap_bench.py needs a HIP device")
    n = 1 << a.log2n
    all_layers = nffacl.ENCAP_VLAN | nffacl.ENCAP_MPLS | nffacl.ENCAP_GRE | nffacl.ENCAP_GTPU
    g = synth.gen_rules(synth.SPECS["c3"], synth.RULE_SEEDS["c3"])
    print(f"c3 imix: {n} frames", file=sys.stderr, flush=True)
    h_frames, h_desc = synth.gen_imix(g, n, synth.PACKET_SEEDS["c3"])
    frames, desc = torch.from_numpy(h_frames).to("cuda"), torch.from_numpy(h_desc.view("int64")).to("cuda")
    del h_frames
    wframes, wdesc = wrap_gtpu(frames, desc)
    del frames, desc
    keys, keys2 = (torch.zeros((n, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    key6, key6_2 = (torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    port, index = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    offsets = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.empty_like(wframes)
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    cap = wframes.numel() // 16 * 16
    with nffacl.Engine(nffacl.L3Rules.parse_text(g.text)) as eng, nffacl.Router(nffacl.ROUTE_SEPARATE, 2, n) as router:
        nffacl.extract_keys_encap_frames_device(wframes, wdesc, n, keys, key6, all_layers, offs)
        eng.classify_keys_device(keys, key6, n, n, port)
        router.route(port, n, index, offsets)
        args = (index, n, out, cap, out_desc, out_bytes, a.align)
        contenders = {"decap": lambda: router.gather_decap_frames(wframes, wdesc, n, offs, keys, *args),
                      "plain": lambda: router.gather_frames(wframes, wdesc, n, *args)}
        if a.alt_lib:  # the same C call into the other build, on a router that build created
            alt = ctypes.CDLL(a.alt_lib)
            handle = ctypes.c_void_p()
            assert alt.nffacl_router_create(0, nffacl.ROUTE_SEPARATE, 2, ctypes.c_uint64(n), ctypes.byref(handle)) == 0
            ptrs = [ctypes.c_void_p(t.data_ptr()) for t in (wframes, wdesc, offs, keys, index, out, out_desc, out_bytes)]
            contenders["alt"] = lambda: alt.nffacl_route_gather_decap_frames_device(
                handle, ptrs[0], ptrs[1], ctypes.c_uint64(n), ptrs[2], ptrs[3], ptrs[4], ctypes.c_uint64(n),
                ctypes.c_uint32(a.align), ptrs[5], ctypes.c_uint64(cap), ptrs[6], ptrs[7], None)
        nbytes, closed = {}, {}
        for name, fn in contenders.items():  # warm-up: code objects, clocks; and the outputs checked below
            out.fill_(0xEE)
            timed(fn, 3)
            torch.cuda.synchronize()
            nbytes[name] = int(out_bytes.cpu()[0])
            assert nbytes[name] <= cap, (name, nbytes[name], cap)
            if name != "plain":
                nffacl.extract_keys_frames_device(out, out_desc, n, keys2, key6_2)
                torch.cuda.synchronize()
                src = index.long()
                six = (keys[src, 3] >> 8) == 6
                k2 = keys2.clone()
                k2[six, 0] = keys[src, 0][six]  # an IPv6 key names its record's place in its own batch
                closed[name] = bool(torch.equal(k2, keys[src]) and torch.equal(key6_2[six], key6[src][six]))
                assert closed[name], f"{name}: the plain keys of the output are not the encap keys"
                del src, six, k2
        times = {name: [] for name in contenders}
        for _ in range(a.rounds):
            for name, fn in contenders.items():
                times[name].append(timed(fn, a.k))
        torch.cuda.synchronize()
        if a.alt_lib:
            alt.nffacl_router_destroy(handle)
    res = {"n": n, "k": a.k, "rounds": a.rounds, "align": a.align, "device": torch.cuda.get_device_name(0),
           "source_bytes": wframes.numel(), "out_bytes": nbytes, "segment_sizes": offsets.cpu().tolist(),
           "output_keys_equal_encap_keys": closed, **{name: summary(xs) for name, xs in times.items()}}
    for name in contenders:
        res[name + "_tbps_read_plus_write"] = (wframes.numel() + nbytes[name]) / res[name]["median_ms"] / 1e9
        if name != "plain":
            res[name + "_over_plain"] = res[name]["median_ms"] / res["plain"]["median_ms"]
            res[name + "_bytes_over_plain"] = (wframes.numel() + nbytes[name]) / (wframes.numel() + nbytes["plain"])
    res["decap_no_slower_than_plain"] = res["decap"]["median_ms"] <= res["plain"]["median_ms"] + max(
        res["decap"]["spread_ms"], res["plain"]["spread_ms"])
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
