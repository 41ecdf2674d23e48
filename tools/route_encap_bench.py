#!/usr/bin/env python3
"""Encapsulating packed-frame gather (csrc/route_encap.hip) on C3's IMIX batch
at n = 2^24 frames, routed SEPARATE by its verdicts, every frame's hop drawn
over a 256-record adjacency table.

  gtpu    Router.gather_encap_frames over the route's whole index, every record
          an 8-byte GTP-U over IPv4 (s = 36, MACS | TTL and the three lengths)
  mix     the same with a table of plain (s = 0), VLAN (4), MPLS (4, 8), GRE
          over IPv4 (24) and GTP-U (36) records
  plain   Router.gather_frames of the same index over the same batch: the
          yardstick
  alt     (--alt-lib) `gtpu` through a second build of the library, e.g. an
          experiment build `make EXTRA=-D... OBJDIR=... OUT=...`

Checked before timing, for every encap contender: extract_keys_encap_frames_device
on the output gives inner_off = 14 + s and the plain keys of the gathered source
frames (those that are IPv4 or IPv6: the batch's 3 % ARP / VLAN frames have no
plain key); checksum_frames_device at cursor 14 finds every GRE / GTP-U outer header
sum right; at the inner cursors the IPv4 header and L4 verdicts are those of the
source frames (the TTL patch kept the header sums).  Each round times K
back-to-back launches between one HIP event pair, the contenders alternating
in this process; the JSON line holds every round's time per launch, medians,
spreads (max - min over the rounds), ratios to `plain`, the bytes each call
reads and writes (source + output, and one 64-byte record per frame for the
encap calls), and whether a median is within plain's times the byte ratio plus
the larger of the two spreads.

usage: python tools/route_encap_bench.py [--log2n 24] [--k 20] [--rounds 7] [--align 64] [--alt-lib LIB.so]
                                         [--out profiles/route_encap/route_encap_bench.json]"""
import argparse
import ctypes
import json
import struct
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "nff-go_amd"), str(ROOT / "tools")]
import nffacl  # noqa: E402
from nffacl import synth  # noqa: E402
from keys_encap_bench import summary, timed  # noqa: E402

IP4H = bytes([0x45, 0, 0, 0, 0, 0, 0, 0, 64, 17, 0, 0, 10, 1, 2, 3, 10, 4, 5, 6])
LEN3 = nffacl.ADJ_IP4_LEN | nffacl.ADJ_UDP_LEN | nffacl.ADJ_GTP_LEN
# (flags, ether_type, shim)
GTPU = (LEN3 | nffacl.ADJ_MACS | nffacl.ADJ_TTL, 0x0800,
        IP4H + struct.pack(">HHHH", 1234, 2152, 0, 0) + bytes([0x30, 255, 0, 0, 0, 0, 0, 9]))
MIX = [(nffacl.ADJ_MACS | nffacl.ADJ_TTL, 0, b""), (nffacl.ADJ_INNER_ETYPE | nffacl.ADJ_MACS, 0x8100, b"\x00\x05\0\0"),
       (nffacl.ADJ_MACS | nffacl.ADJ_TTL, 0x8847, b"\x00\x01\x01\x40"),
       (nffacl.ADJ_MACS, 0x8847, b"\x00\x01\x00\x40\x00\x01\x11\x40"),
       (nffacl.ADJ_IP4_LEN | nffacl.ADJ_INNER_ETYPE | nffacl.ADJ_MACS | nffacl.ADJ_TTL, 0x0800,
        IP4H[:9] + b"\x2f" + IP4H[10:] + b"\0\0\0\0"), GTPU]


def table(kinds, count=256):
    adj = np.zeros(count, nffacl.ADJ_DTYPE)
    for k in range(count):
        fl, et, shim = kinds[k % len(kinds)]
        adj["flags"][k], adj["ether_type"][k], adj["shim_len"][k] = fl, et, len(shim)
        adj["shim"][k, :len(shim)] = np.frombuffer(shim, np.uint8)
        adj["dmac"][k], adj["smac"][k] = (2, 0, 0, 0, 1, k), (2, 0, 0, 0, 0, k & 7)
    return adj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--align", type=int, default=64)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "route_encap" / "route_encap_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("route_encap_bench.py needs a HIP device")
    n = 1 << a.log2n
    all_layers = nffacl.ENCAP_VLAN | nffacl.ENCAP_MPLS | nffacl.ENCAP_GRE | nffacl.ENCAP_GTPU
    g = synth.gen_rules(synth.SPECS["c3"], synth.RULE_SEEDS["c3"])
    print(f"c3 imix: {n} frames", file=sys.stderr, flush=True)
    h_frames, h_desc = synth.gen_imix(g, n, synth.PACKET_SEEDS["c3"])
    frames, desc = torch.from_numpy(h_frames).to("cuda"), torch.from_numpy(h_desc.view("int64")).to("cuda")
    del h_frames
    tables = {"gtpu": table([GTPU]), "mix": table(MIX)}
    d_adj = {k: torch.from_numpy(t.view(np.uint8)).to("cuda") for k, t in tables.items()}
    hop = torch.randint(0, 256, (n,), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(7))
    keys, keys2 = (torch.zeros((n, 4), dtype=torch.int32, device="cuda") for _ in range(2))
    key6, key6_2 = (torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    port, index = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    offsets = torch.zeros(4, dtype=torch.int32, device="cuda")
    sums, sums_src = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cap = int((((desc & 0xFFFF) + 36 + a.align - 1) // a.align * a.align).sum())
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    with nffacl.Engine(nffacl.L3Rules.parse_text(g.text)) as eng, nffacl.Router(nffacl.ROUTE_SEPARATE, 2, n) as router:
        nffacl.extract_keys_frames_device(frames, desc, n, keys, key6)
        nffacl.checksum_frames_device(frames, desc, n, sums_src)
        eng.classify_keys_device(keys, key6, n, n, port)
        router.route(port, n, index, offsets)
        args = (index, n, out, cap, out_desc, out_bytes)
        contenders = {"gtpu": lambda: router.gather_encap_frames(frames, desc, n, hop, d_adj["gtpu"], 256, *args, status,
                                                                 a.align),
                      "mix": lambda: router.gather_encap_frames(frames, desc, n, hop, d_adj["mix"], 256, *args, status,
                                                                a.align),
                      "plain": lambda: router.gather_frames(frames, desc, n, *args, a.align)}
        if a.alt_lib:  # the same C call into the other build, on a router that build created
            alt = ctypes.CDLL(a.alt_lib)
            handle = ctypes.c_void_p()
            assert alt.nffacl_router_create(0, nffacl.ROUTE_SEPARATE, 2, ctypes.c_uint64(n), ctypes.byref(handle)) == 0
            ptrs = [ctypes.c_void_p(t.data_ptr()) for t in (frames, desc, hop, d_adj["gtpu"], index, out, out_desc,
                                                            out_bytes, status)]
            contenders["alt"] = lambda: alt.nffacl_route_gather_encap_frames_device(
                handle, ptrs[0], ptrs[1], ctypes.c_uint64(n), ptrs[2], ptrs[3], ctypes.c_uint32(256), ptrs[4],
                ctypes.c_uint64(n), ctypes.c_uint32(a.align), ptrs[5], ctypes.c_uint64(cap), ptrs[6], ptrs[7], ptrs[8],
                None)
        nbytes, closed, src = {}, {}, index.long()
        bad = nffacl.CK_IP4_BAD | nffacl.CK_L4_BAD
        for name, fn in contenders.items():  # warm-up: code objects, clocks; and the outputs checked below
            out.fill_(0xEE)
            timed(fn, 3)
            torch.cuda.synchronize()
            nbytes[name] = int(out_bytes.cpu()[0])
            assert nbytes[name] <= cap, (name, nbytes[name], cap)
            if name != "plain":
                s = torch.from_numpy(tables["mix" if name == "mix" else "gtpu"]["shim_len"].astype(np.int64)).to("cuda")
                s = s[hop.long()[src]]
                nffacl.extract_keys_encap_frames_device(out, out_desc, n, keys2, key6_2, all_layers, offs)
                nffacl.checksum_frames_device(out, out_desc, n, sums, what=nffacl.CK_IP4)
                torch.cuda.synchronize()
                fam = keys[src, 3] >> 8
                ip, six = fam != 0, fam == 6  # synth's 3 % ARP / VLAN frames have no plain key to close with
                k2 = keys2.clone()
                k2[six, 0] = keys[src, 0][six]  # an IPv6 key names its record's place in its own batch
                outer = (sums >> 32)[s >= 24] & (nffacl.CK_IP4_DONE | nffacl.CK_IP4_BAD)
                ok = [torch.equal(offs.long()[ip], 14 + s[ip]), torch.equal(k2[ip], keys[src][ip]),
                      torch.equal(key6_2[six], key6[src][six]), bool((outer == nffacl.CK_IP4_DONE).all())]
                nffacl.checksum_frames_device(out, out_desc, n, sums, inner_off=offs)
                torch.cuda.synchronize()
                ok.append(torch.equal(((sums >> 32) & bad)[ip], ((sums_src[src] >> 32) & bad)[ip]))
                closed[name] = ok
                assert all(ok), f"{name}: the output does not close with the keys and checksums: {ok}"
                del s, six, k2, outer
        times = {name: [] for name in contenders}
        for _ in range(a.rounds):
            for name, fn in contenders.items():
                times[name].append(timed(fn, a.k))
        torch.cuda.synchronize()
        if a.alt_lib:
            alt.nffacl_router_destroy(handle)
    res = {"n": n, "k": a.k, "rounds": a.rounds, "align": a.align, "device": torch.cuda.get_device_name(0),
           "source_bytes": frames.numel(), "out_bytes": nbytes, "segment_sizes": offsets.cpu().tolist(),
           "output_closes": closed, **{name: summary(xs) for name, xs in times.items()}}
    moved = {name: frames.numel() + nbytes[name] + (64 * n if name != "plain" else 0) for name in contenders}
    for name in contenders:
        res[name + "_tbps_read_plus_write"] = moved[name] / res[name]["median_ms"] / 1e9
        if name != "plain":
            res[name + "_over_plain"] = res[name]["median_ms"] / res["plain"]["median_ms"]
            res[name + "_bytes_over_plain"] = moved[name] / moved["plain"]
            res[name + "_within_bar"] = res[name]["median_ms"] <= res["plain"]["median_ms"] * moved[name] / moved[
                "plain"] + max(res[name]["spread_ms"], res["plain"]["spread_ms"])
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
