#!/usr/bin/env python3
"""Keys of encapsulated frames (csrc/keys_encap.hip) on C3's IMIX batch at
n = 2^24 frames, once as it is and once with every frame wrapped in 8-byte
GTP-U over IPv4 (36 bytes of shims, DecapsulateIPv4GTP's shape):

  plain    extract_keys_frames_device on the plain batch (the yardstick)
  offered  extract_keys_encap_frames_device, every layer enabled, on the plain
           batch: what merely offering the resolution costs
  wrapped  the same call on the wrapped batch

Outputs are compared first: the wrapped batch's keys must be the plain
batch's plain keys wherever those are IPv4 or IPv6 (the batch's ARP and
tagged frames have no version nibble for GTP-U to go by), its cursors 50;
whether the plain batch gives the same keys with every layer enabled is
recorded (its tagged frames resolve to their inner headers then).  Each
round times K back-to-back launches between one HIP event pair, the three
contenders alternating in this process; the JSON line holds every round's
time per launch, the medians, the spreads (max - min over the rounds) and the
ratios to `plain`.

usage: python tools/keys_encap_bench.py [--log2n 24] [--k 20] [--rounds 7]
                                        [--out profiles/keys_encap/keys_encap_bench.json]"""
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

SHIM = bytes([0x45, 0, 0, 0, 0, 0, 0, 0, 64, 17, 0, 0, 10, 1, 2, 3, 10, 4, 5, 6,  # IPv4, protocol UDP
              0x08, 0x68, 0x08, 0x68, 0, 0, 0, 0,                                # UDP 2152 -> 2152
              0x30, 255, 0, 0, 0, 0, 0, 9])                                      # GTPv1, PT 1, G-PDU, TEID 9


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


def wrap_gtpu(frames, desc, chunk=1 << 20):
    """The batch with SHIM inserted at byte 14 of every frame and the EtherType set to IPv4, packed at 64-byte
    rooms.  A frame's first 128 bytes carry its headers (synth.gen_imix), the rest is zero payload."""
    n, t = desc.numel(), len(SHIM)
    lens = (desc & 0xFFFF) + t
    room = (lens + 63) // 64 * 64
    offs = torch.cumsum(room, 0) - room
    out = torch.zeros(int(offs[-1] + room[-1]) + 128, dtype=torch.uint8, device=frames.device)
    rows, src = out[:out.numel() // 64 * 64].view(-1, 64), frames[:frames.numel() // 64 * 64].view(-1, 64)
    shim = torch.tensor(list(b"\x08\x00" + SHIM), dtype=torch.uint8, device=frames.device)
    col = torch.arange(192, device=frames.device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        line, ln = desc[c0:c1] >> 22, desc[c0:c1] & 0xFFFF
        head = src[line[:, None] + torch.arange(2, device=frames.device)].reshape(-1, 128)
        head = head * (col[:128] < ln[:, None])  # a short frame's second line is its neighbour's
        img = torch.zeros((c1 - c0, 192), dtype=torch.uint8, device=frames.device)
        img[:, :12], img[:, 12:14 + t], img[:, 14 + t:128 + t] = head[:, :12], shim, head[:, 14:]
        img = (img * (col < lens[c0:c1, None])).view(-1, 3, 64)
        dst = offs[c0:c1] >> 6
        for j in range(3):
            m = room[c0:c1] > 64 * j  # never touch the next frame's room
            rows[dst[m] + j] = img[m, j]
    return out, offs << 16 | lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keys_encap" / "keys_encap_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("keys_encap_bench.py needs a HIP device")
    n = 1 << a.log2n
    all_layers = nffacl.ENCAP_VLAN | nffacl.ENCAP_MPLS | nffacl.ENCAP_GRE | nffacl.ENCAP_GTPU
    g = synth.gen_rules(synth.SPECS["c3"], synth.RULE_SEEDS["c3"])
    print(f"c3 imix: {n} frames", file=sys.stderr, flush=True)
    h_frames, h_desc = synth.gen_imix(g, n, synth.PACKET_SEEDS["c3"])
    frames, desc = torch.from_numpy(h_frames).to("cuda"), torch.from_numpy(h_desc.view("int64")).to("cuda")
    del h_frames
    wframes, wdesc = wrap_gtpu(frames, desc)
    keys, keys_o, keys_w = (torch.zeros((n, 4), dtype=torch.int32, device="cuda") for _ in range(3))
    key6, key6_w = (torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    contenders = {
        "plain": lambda: nffacl.extract_keys_frames_device(frames, desc, n, keys, key6),
        "offered": lambda: nffacl.extract_keys_encap_frames_device(frames, desc, n, keys_o, key6, all_layers),
        "wrapped": lambda: nffacl.extract_keys_encap_frames_device(wframes, wdesc, n, keys_w, key6_w, all_layers, offs),
    }
    for fn in contenders.values():
        timed(fn, 3)  # warm-up: code objects, clocks; and the outputs compared below
    torch.cuda.synchronize()
    fam = keys[:, 3] >> 8
    assert torch.equal(keys_w[fam != 0], keys[fam != 0]) and torch.equal(key6_w[fam == 6], key6[fam == 6]) and \
        bool((offs == 14 + len(SHIM)).all()), "the wrapped batch's keys are not the plain batch's"
    offered_equal = bool(torch.equal(keys_o, keys))
    times = {name: [] for name in contenders}
    for _ in range(a.rounds):
        for name, fn in contenders.items():
            times[name].append(timed(fn, a.k))
    res = {"n": n, "k": a.k, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "plain_bytes": frames.numel(), "wrapped_bytes": wframes.numel(), "wrapped_keys_equal_plain_keys": True,
           "offered_keys_equal_plain_keys": offered_equal, **{name: summary(xs) for name, xs in times.items()}}
    for name in ("offered", "wrapped"):
        res[name + "_over_plain"] = res[name]["median_ms"] / res["plain"]["median_ms"]
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
