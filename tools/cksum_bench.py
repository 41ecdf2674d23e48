#!/usr/bin/env python3
"""Checksums of packed frames (csrc/cksum.hip) on C3's IMIX batch at n = 2^24
frames.  The synthetic frames are headers over zero payload, and not every one
has an L4 span that covers it: `cover` first rewrites the header fields on the
device so that every frame is IPv4 (IHL 5) or IPv6 with TCP, UDP or ICMP whose
TotalLength / PayloadLen (and DgramLen) reach the frame's end — the 3 % of
non-IP frames become IPv4 / UDP, a TCP span under 20 bytes becomes UDP.  It is
checked over the whole batch that L4_DONE is set everywhere: otherwise the
kernel reads nothing and the number is void.

  full    checksum_frames_device, what = CK_IP4 | CK_L4
  ip4     checksum_frames_device, what = CK_IP4 (one line per frame)
  gather  Router.gather_frames with the identity index over the same batch:
          the bar; it reads and writes the bytes `full` only reads
  keys    extract_keys_frames_device: the same one-line-per-frame pass as ip4

Each round times K back-to-back launches between one HIP event pair, the
contenders alternating in this process; the JSON line holds every round's time
per launch, the medians, the spreads (max - min over the rounds), the read
rates over the frames' bytes, full / gather with the bar's verdict, and
ip4 / keys (no bar).

usage: python tools/cksum_bench.py [--log2n 24] [--k 20] [--rounds 7] [--out profiles/cksum/cksum_bench.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "nff-go_amd"), str(ROOT / "tools")]
import nffacl  # noqa: E402
from nffacl import synth  # noqa: E402
from keys_encap_bench import summary, timed  # noqa: E402


def cover(frames, desc):
    """Rewrite the header fields of every frame (in place) so that its L4 span is [34 or 54, length)."""
    off, ln = desc >> 16, desc & 0xFFFF

    def put16(at, v):
        frames[at], frames[at + 1] = (v >> 8).to(torch.uint8), (v & 255).to(torch.uint8)

    six = (frames[off + 12] == 0x86) & (frames[off + 13] == 0xDD)
    four = ~six
    other = four & ~((frames[off + 12] == 0x08) & (frames[off + 13] == 0x00))
    o4 = off[four]
    frames[o4 + 12], frames[o4 + 13], frames[o4 + 14] = 0x08, 0x00, 0x45
    put16(o4 + 16, ln[four] - 14)
    frames[o4 + 20], frames[o4 + 21] = 0, 0
    b = torch.where(six, 54, 34)
    m, at = ln - b, off + torch.where(six, 20, 23)  # the span's bytes, where the protocol is
    p = frames[at].long()
    ok = ((p == 6) & (m >= 20)) | (p == 17) | (p == torch.where(six, 58, 1))
    p = torch.where(ok & ~other, p, 17)
    frames[at] = p.to(torch.uint8)
    put16(off[six] + 18, m[six])
    udp = p == 17
    put16((off + b)[udp] + 4, m[udp])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cksum" / "cksum_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cksum_bench.py needs a HIP device")
    n = 1 << a.log2n
    g = synth.gen_rules(synth.SPECS["c3"], synth.RULE_SEEDS["c3"])
    print(f"c3 imix: {n} frames", file=sys.stderr, flush=True)
    h_frames, h_desc = synth.gen_imix(g, n, synth.PACKET_SEEDS["c3"])
    frames, desc = torch.from_numpy(h_frames).to("cuda"), torch.from_numpy(h_desc.view("int64")).to("cuda")
    del h_frames
    cover(frames, desc)
    frame_bytes = int((desc & 0xFFFF).sum())
    sums = torch.zeros(n, dtype=torch.int64, device="cuda")
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    keys, key6 = (torch.zeros((n, k), dtype=torch.int32, device="cuda") for k in (4, 8))
    index = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.empty_like(frames)
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    cap = frames.numel() // 16 * 16
    with nffacl.Router(nffacl.ROUTE_SEPARATE, 2, n) as router:
        contenders = {
            "full": lambda: nffacl.checksum_frames_device(frames, desc, n, sums, bits),
            "ip4": lambda: nffacl.checksum_frames_device(frames, desc, n, sums, bits, what=nffacl.CK_IP4),
            "gather": lambda: router.gather_frames(frames, desc, n, index, n, out, cap, out_desc, out_bytes, 64),
            "keys": lambda: nffacl.extract_keys_frames_device(frames, desc, n, keys, key6)}
        contenders["full"]()
        torch.cuda.synchronize()
        status = sums >> 32
        done = int(((status & nffacl.CK_L4_DONE) != 0).sum())
        assert done == n, f"L4_DONE on {done} of {n} frames: the batch is not covered"
        ip4_done = int(((status & nffacl.CK_IP4_DONE) != 0).sum())
        del status
        for fn in contenders.values():  # warm-up: code objects, clocks
            timed(fn, 3)
        times = {name: [] for name in contenders}
        for _ in range(a.rounds):
            for name, fn in contenders.items():
                times[name].append(timed(fn, a.k))
        torch.cuda.synchronize()
        gathered = int(out_bytes.cpu()[0])
    res = {"n": n, "k": a.k, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "batch_bytes": frames.numel(), "frame_bytes": frame_bytes, "l4_done": done, "ip4_done": ip4_done,
           "gather_out_bytes": gathered, **{name: summary(xs) for name, xs in times.items()}}
    res["full_tbps_read"] = frame_bytes / res["full"]["median_ms"] / 1e9
    res["gather_tbps_read_plus_write"] = (frame_bytes + gathered) / res["gather"]["median_ms"] / 1e9
    res["full_over_gather"] = res["full"]["median_ms"] / res["gather"]["median_ms"]
    res["full_no_slower_than_gather"] = res["full"]["median_ms"] <= res["gather"]["median_ms"]
    res["ip4_over_keys"] = res["ip4"]["median_ms"] / res["keys"]["median_ms"]
    line = json.dumps(res)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
