"""Checksums of packed frames (csrc/cksum.hip), exact against a numpy reference written from nffacl.h."""
import functools
import json
import struct
from pathlib import Path

import numpy as np
import pytest

import nffacl
from nffacl import CK_FRAGMENT, CK_IP4, CK_IP4_BAD, CK_IP4_DONE, CK_L4, CK_L4_ABSENT, CK_L4_BAD, CK_L4_DONE, CK_LENGTH
from test_route_decap import ALL, SHIMS  # the shim table of the decapsulating gather's test

T = -(-(1 << 20) // nffacl.checksum_frames_plan(1 << 20))  # frames per tile
BOTH = CK_IP4 | CK_L4
KATS = json.loads((Path(__file__).parent / "golden" / "checksum_kats.json").read_text())


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def words(x):  # the sum of the big-endian words of x, an odd last byte padded with 0 on the right
    return int(np.append(x, np.zeros(len(x) & 1, np.uint8)).view(">u2").astype(np.uint64).sum())


def fold(s):  # reduceChecksum
    return s if s <= 0xFFFF else fold((s >> 16) + (s & 0xFFFF))


def reference(f, c=14, what=BOTH):
    """(ip, l4, status) of one frame (uint8[L]) at cursor c, as nffacl.h defines them."""
    L, be = len(f), lambda o: int(f[o]) << 8 | int(f[o + 1])
    if c & 1 or c < 14 or c >= L:
        return 0, 0, 0
    fam, ip, st = int(f[c]) >> 4, 0, 0
    if fam not in (4, 6) or (c == 14 and be(12) != {4: 0x0800, 6: 0x86DD}[fam]) or (fam == 6 and not what & CK_L4):
        return 0, 0, 0
    if fam == 4:
        H = 4 * (int(f[c]) & 15)
        if H < 20 or c + H > L:
            return 0, 0, CK_LENGTH
        if what & CK_IP4:
            h = f[c:c + H].copy()
            h[10:12] = 0
            ip, st = ~fold(words(h)) & 0xFFFF, CK_IP4_DONE
            st |= 0 if (ip or 0xFFFF) == (be(c + 10) or 0xFFFF) else CK_IP4_BAD
        if not what & CK_L4:
            return ip, 0, st
        if be(c + 2) < H or c + be(c + 2) > L:
            return ip, 0, st | CK_LENGTH
        if be(c + 6) & 0x3FFF:
            return ip, 0, st | CK_FRAGMENT
        proto, b, e, icmp, pseudo = int(f[c + 9]), c + H, c + be(c + 2), 1, words(f[c + 12:c + 20])
    else:
        if c + 40 > L or c + 40 + be(c + 4) > L:
            return 0, 0, CK_LENGTH
        proto, b, e, icmp, pseudo = int(f[c + 6]), c + 40, c + 40 + be(c + 4), 58, words(f[c + 8:c + 40])
    if proto not in (6, 17, icmp):
        return ip, 0, st
    m, at = e - b, {6: 16, 17: 6}.get(proto, 2)
    if m < (20 if proto == 6 else 8) or (proto == 17 and be(b + 4) != m):
        return ip, 0, st | CK_LENGTH
    s = f[b:e].copy()
    s[at:at + 2] = 0
    l4 = ~fold(words(s) + (0 if (fam, proto) == (4, 1) else pseudo + proto + m)) & 0xFFFF
    l4, stored = (0xFFFF if proto == 17 and l4 == 0 else l4), be(b + at)
    if proto == 17 and stored == 0:
        return ip, l4, st | CK_L4_DONE | (CK_L4_ABSENT if fam == 4 else CK_L4_BAD)
    return ip, l4, st | CK_L4_DONE | (0 if (l4 or 0xFFFF) == (stored or 0xFFFF) else CK_L4_BAD)


def packet(rng, six, proto, m, ihl=5, pad=0):
    """A random frame with its checksums written in: IPv4 (ihl) or IPv6, L4 `proto` of 0 TCP / 1 UDP / 2 ICMP and m
    bytes, `pad` bytes of Ethernet padding; returns (frame, offset of L4, offset of its checksum field)."""
    b, p = 14 + (40 if six else 4 * ihl), (6, 17, 58 if six else 1)[proto]
    f, at = np.frombuffer(rng.bytes(b + m + pad), np.uint8).copy(), b + (16, 6, 2)[proto]
    f[12:14] = (0x86, 0xDD) if six else (0x08, 0x00)
    if six:
        f[14], f[18:20], f[20] = 0x60 | f[14] & 15, (m >> 8, m & 255), p
    else:
        f[14], f[16:18], f[20:22], f[23] = 0x40 | ihl, ((b - 14 + m) >> 8, (b - 14 + m) & 255), (f[20] & 0x40, 0), p
    if p == 17:
        f[b + 4:b + 6] = m >> 8, m & 255
    ip, l4, _ = reference(f)
    f[at:at + 2] = l4 >> 8, l4 & 255
    if not six:
        f[24:26] = ip >> 8, ip & 255
    return f, b, at


def pack(fs):  # frames in 16-byte rooms, 0xA5 past each length, the buffer sized exactly; descriptors
    ln = np.array([len(f) for f in fs], np.int64)
    off = np.cumsum((ln + 15) // 16 * 16) - (ln + 15) // 16 * 16
    buf = np.full(int(((ln + 15) // 16 * 16).sum()), 0xA5, np.uint8)
    for f, o in zip(fs, off):
        buf[o:o + len(f)] = f
    return buf, (off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64))


@functools.lru_cache(maxsize=None)
def batch(n):
    """n frames, IHL 5-15, lengths 15-1518, spans of 8 bytes to 90 chunks: by i % 20 intact (padded after
    TotalLength every third time) or one of the cases below; with their descriptors."""
    rng, out = np.random.default_rng(1000 + n), []
    for i in range(n):
        k, six, proto = i % 20, bool(rng.integers(2)), int(rng.integers(3))
        m = int(rng.integers((20, 8, 8)[proto], 1434)) if rng.random() < 0.5 else int(rng.integers(20, 64))
        f, b, at = packet(rng, six and k not in (1, 7, 9, 10), 1 if k in (8, 11, 12) else proto, 8 if k == 12 else m,
                          int(rng.integers(5, 16)), int(rng.integers(0, 12)) if k % 3 == 0 else 0)
        if k in (2, 5):    # a span byte spoiled (pad bytes are not in the span)
            f[int(rng.integers(b, b + m))] ^= int(rng.integers(1, 256))
        elif k == 1:       # an IPv4 header byte spoiled
            f[int(rng.integers(14, b))] ^= int(rng.integers(1, 256))
        elif k == 7:       # an IPv4 header that sums to 0xFFFF, stored as 0xFFFF
            f[18:20] = f[24:26] = 0
            s = 0xFFFF - fold(words(f[14:b]))
            f[18:20], f[24:26] = (s >> 8, s & 255), (0xFF, 0xFF)
        elif k == 8:       # UDP sent without a checksum, either family
            f[at:at + 2] = 0
        elif k == 9:       # a fragment: MF, or an offset
            f[20:22] = (0x20, 0) if i & 32 else (0, 3)
        elif k == 10:      # TotalLength below the header
            f[16:18] = 0, b - 14 - 4
        elif k == 11:      # DgramLen != m
            f[b + 5] ^= 1
        elif k == 13:      # TotalLength / PayloadLen past the frame
            f = f[:len(f) - int(rng.integers(1, 8))]
        elif k == 14:      # a cut header
            f = f[:15 if i == 14 else int(rng.integers(15, b))]
        elif k == 16:      # ARP, or IPv6 with a hop-by-hop header
            f[12:14], f[20] = ((0x86, 0xDD), 0) if six else ((0x08, 0x06), f[20])
        elif k == 17:      # EtherType and version nibble disagree
            f[14] ^= 0x20
        elif k == 19:      # TCP below its minimum
            f, b, at = packet(rng, six, 0, 20)
            f[18 if six else 16:20 if six else 18] = 0, 12 if six else b - 14 + 12
        out.append(f)
    return pack(out)


@functools.lru_cache(maxsize=None)
def wanted(n, what):  # the reference's records for batch(n)
    buf, desc = batch(n)
    return np.array([reference(buf[d >> 16:(d >> 16) + (d & 0xFFFF)], 14, what) for d in desc.astype(np.int64)],
                    np.int64).reshape(n, 3)


def run(torch, buf, desc, what=BOTH, inner_off=None, n=None):  # (ip, l4, status)[n], bad bits; both guards checked
    n = len(desc) if n is None else n
    words64 = (n + 63) // 64
    dev = [torch.from_numpy(a).to("cuda") for a in (buf, desc.view(np.int64))]
    off = None if inner_off is None else torch.from_numpy(np.asarray(inner_off, np.uint16).view(np.int16)).to("cuda")
    sums, bits = (torch.full((k + 2,), -1, dtype=torch.int64, device="cuda") for k in (n, words64))
    nffacl.checksum_frames_device(dev[0], dev[1], n, sums, bits, off, what)
    torch.cuda.synchronize()
    sums, bits = sums.cpu().numpy(), bits.cpu().numpy()
    assert (sums[n:] == -1).all() and (bits[words64:] == -1).all()
    rec = sums[:n].view(nffacl.CKSUM_DTYPE)
    return np.stack([rec["ip"], rec["l4"], rec["status"]], 1).astype(np.int64), bits[:words64].view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("what", [CK_IP4, CK_L4, BOTH])
@pytest.mark.parametrize("n", [0, 1, 63, 65, T + 1, 2 * T + 37])
def test_checksums_match_reference(torch, n, what):
    (buf, desc), want = batch(n), wanted(n, what)
    if n >= 65:  # (on the inputs) every status bit and the all-zero record occur; the extreme lengths at T + 1
        st = wanted(n, BOTH)[:, 2]
        assert all((st & bit).any() for bit in (1, 2, 4, 8, 16, 32, 64)) and (wanted(n, BOTH).sum(1) == 0).any()
        assert n < T or ((desc & np.uint64(0xFFFF)).min() == 15 and (desc & np.uint64(0xFFFF)).max() > 1400)
    if n == 0:  # (an empty tensor has no address)
        buf, desc = np.zeros(16, np.uint8), np.zeros(1, np.uint64)
    got, bits = run(torch, buf, desc, what, n=n)
    np.testing.assert_array_equal(got, want)
    bad = np.zeros(len(bits) * 64, bool)
    bad[:n] = (want[:, 2] & (CK_IP4_BAD | CK_L4_BAD)) != 0
    np.testing.assert_array_equal(bits, np.packbits(bad, bitorder="little").view(np.uint64))


@pytest.mark.gpu
def test_cursors_reach_the_inner_checksums(torch):
    rng, wires, n = np.random.default_rng(23), [], 54
    for i in range(n):  # every shim around IPv4 and IPv6 with TCP, UDP and ICMP, checksums valid
        f, (outer, shim) = packet(rng, i % 2 == 1, i // 2 % 3, 46 + i)[0].tobytes(), SHIMS[i % len(SHIMS)]
        wires.append(np.frombuffer(f[:12] + (struct.pack(">H", outer) if outer else f[12:14]) +
                                   shim.replace(b"<>", f[12:14]) + f[14:], np.uint8))
    buf, desc = pack(wires)
    frames_d, desc_d = torch.from_numpy(buf).to("cuda"), torch.from_numpy(desc.view(np.int64)).to("cuda")
    keys, key6 = (torch.zeros((n, k), dtype=torch.int32, device="cuda") for k in (4, 8))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    out = torch.zeros(len(buf) + 64 * n, dtype=torch.uint8, device="cuda")
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, n) as r:
        nffacl.extract_keys_encap_frames_device(frames_d, desc_d, n, keys, key6, ALL, offs)
        r.gather_decap_frames(frames_d, desc_d, n, offs, keys, torch.arange(n, dtype=torch.int32, device="cuda"), n,
                              out, out.numel(), out_desc, out_bytes)
        torch.cuda.synchronize()
    cur = offs.cpu().numpy().view(np.uint16)
    inner = run(torch, buf, desc, inner_off=cur)[0]
    assert (inner[:, 2] & CK_L4_DONE).all() and not (inner[:, 2] & (CK_IP4_BAD | CK_L4_BAD)).any()
    plain = run(torch, out.cpu().numpy(), out_desc.cpu().numpy().view(np.uint64))[0]
    np.testing.assert_array_equal(plain[:, :2], inner[:, :2])
    for c in (cur[:3] + 1, np.full(3, 0xFFFF), desc[:3] & np.uint64(0xFFFF)):  # odd, malformed, at the frame's end
        assert not run(torch, buf, desc[:3], inner_off=c)[0].any()


def test_reference_gives_the_known_answers():
    got = [reference(np.frombuffer(bytes.fromhex(k["frame"]), np.uint8))[int(k["field"] == "l4")] for k in KATS]
    assert len(KATS) == 7 and [hex(g) for g in got] == [k["want"] for k in KATS]


@pytest.mark.gpu
def test_kernel_gives_the_known_answers(torch):
    got = run(torch, *pack([np.frombuffer(bytes.fromhex(k["frame"]), np.uint8) for k in KATS]))[0]
    assert [hex(g[int(k["field"] == "l4")]) for g, k in zip(got, KATS)] == [k["want"] for k in KATS]


@pytest.mark.gpu
@pytest.mark.parametrize("arg,value", [(6, 0), (6, 4), (6, 7), (3, None), (0, None), (0, 8), (1, None), (1, 4), (5, 1),
                                       (3, 4), (4, 4), (2, 1 << 32)])
def test_bad_arguments_are_refused(torch, arg, value):  # what; both outputs NULL; NULL, misaligned buffers; n
    sums, bits = (torch.full((k,), -1, dtype=torch.int64, device="cuda") for k in (65, 2))
    good = [*(torch.from_numpy(a).to("cuda") for a in (batch(65)[0], batch(65)[1].view(np.int64))), 65, sums, bits,
            torch.full((65,), 14, dtype=torch.int16, device="cuda"), BOTH]
    if arg == 3 and value is None:
        good[4] = None
    elif value is not None and arg not in (2, 6):
        value += good[arg].data_ptr()
    with pytest.raises(nffacl.NFError) as e:
        nffacl.checksum_frames_device(*good[:arg], value, *good[arg + 1:])
    torch.cuda.synchronize()
    assert e.value.status == nffacl.ERR_INVALID_ARG
    assert (sums.cpu().numpy() == -1).all() and (bits.cpu().numpy() == -1).all()  # no launch


def test_plan():
    for n in (0, 1, T, T + 1, (1 << 32) - 1):
        tiles = nffacl.checksum_frames_plan(n)
        assert tiles >= 1 and tiles * -(-n // tiles) >= n and -(-n // tiles) <= T
    with pytest.raises(nffacl.NFError):
        nffacl.checksum_frames_plan(1 << 32)
