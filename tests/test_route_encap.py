"""Encapsulating packed-frame gather (csrc/route_encap.hip), exact against a numpy packing written from nffacl.h."""
import struct

import numpy as np
import pytest

import nffacl
from nffacl import (ADJ_GTP_LEN as GTP, ADJ_INNER_ETYPE as INNER, ADJ_IP4_LEN as IP4, ADJ_MACS as MACS, ADJ_TTL as TTL,
                    ADJ_UDP_LEN as UDP)
from test_route_decap import ALL, GTPU, IP4 as IP4H, T, indices, torch  # noqa: F401  (torch: the device fixture)

# (shim_len, flags, ether_type): every s % 16, s >= 16, the maximum, the flag sets each length allows; the last two
# are malformed (s = 6; GTP_LEN with s = 28) and must leave their frames alone
RECORDS = [(0, 0, 0), (0, MACS | TTL, 0x8100), (4, INNER | MACS, 0x8100), (4, TTL, 0x8847), (8, INNER | TTL, 0x88A8),
           (8, MACS, 0), (12, MACS | TTL, 0x8847), (16, INNER, 0), (16, MACS | TTL, 0x8847),
           (20, IP4 | INNER | TTL, 0x0800), (20, IP4 | MACS, 0x0800), (24, IP4 | INNER | MACS | TTL, 0x0800),
           (28, IP4 | UDP | TTL, 0x0800), (36, 63, 0x0800), (36, IP4 | UDP | GTP | MACS | TTL, 0x0800), (36, 0, 0x0800),
           (48, IP4 | UDP | GTP | TTL, 0x0800), (48, MACS | INNER, 0), (6, MACS, 0x8100), (28, IP4 | UDP | GTP, 0x0800)]


def csum(b):  # ~reduceChecksum of the big-endian words of b
    s = int(np.frombuffer(bytes(b) + bytes(len(b) % 2), ">u2").sum(dtype=np.uint64))
    while s > 0xFFFF:
        s = (s >> 16) + (s & 0xFFFF)
    return ~s & 0xFFFF


def table(records, seed):  # ADJ_DTYPE records with random MACs and shim templates
    rng = np.random.default_rng(seed)
    adj = np.zeros(len(records), nffacl.ADJ_DTYPE)
    adj["shim_len"], adj["flags"], adj["ether_type"] = np.array(records).T
    for k in ("dmac", "smac", "shim"):
        adj[k] = rng.integers(0, 256, adj[k].shape)
    return adj


def batch(n, seed):
    """n frames in 16-byte rooms (0xA5 past each length, the buffer sized exactly): a third with an IPv4 header at 14
    (TTL of {0, 1, 2, 64, 255}, IHL 5 or 6), a tenth IPv6 (hop limit of {0, 1, 2, 64}), the rest random bytes;
    lengths around every threshold and two near 65535; descriptors; hops over RECORDS with about 5 % past the table
    and noise above bit 24."""
    rng = np.random.default_rng(seed)
    edge = [0, 13, 14, 15, 16, 17, 31, 32, 33, 34, 35, 53, 54]
    ln = np.where(rng.random(n) < 0.3, rng.choice(edge, n), rng.integers(15, 1519, n))
    ln[5:7] = [65500, 65530][:len(ln[5:7])]
    room = (ln + 15) // 16 * 16
    off = np.cumsum(room) - room
    frames = rng.integers(0, 256, int(room.sum()), dtype=np.uint8)
    kind = rng.random(n)
    for i in np.flatnonzero((kind < 0.43) & (ln >= 23)):
        o, v4 = off[i], kind[i] < 0.33
        frames[o + 12:o + 15] = (0x08, 0x00, 0x40 | rng.choice([5, 6])) if v4 else (0x86, 0xDD, 0x60 | rng.integers(16))
        frames[o + (22 if v4 else 21)] = rng.choice([0, 1, 2, 64, 255] if v4 else [0, 1, 2, 64])
    frames[np.arange(len(frames)) - np.repeat(off, room) >= np.repeat(ln, room)] = 0xA5
    hop = np.where(rng.random(n) < 0.05, rng.choice([len(RECORDS), len(RECORDS) + 7, 0xFFFFFF], n),
                   rng.integers(0, len(RECORDS), n)) | rng.integers(0, 256, n) << 24
    return frames, off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64), hop.astype(np.uint32)


def rewrite(f, A):  # (bytes, status) of one source frame under record A, as nffacl.h defines it
    L, s, fl = len(f), int(A["shim_len"]), int(A["flags"])
    ok = L >= 14 and s % 4 == 0 and s <= 48 and fl < 64 and L + s <= 65535
    ok = ok and all(s >= least for bit, least in ((INNER, 4), (IP4, 20), (UDP, 28), (GTP, 36)) if fl & bit)
    if not (ok and (not fl & UDP or fl & IP4) and (not fl & GTP or fl & UDP)):
        return f, 0
    shim, inner, st = bytearray(A["shim"][:s].tobytes()), bytearray(f[14:]), nffacl.RW_APPLIED
    if fl & INNER:
        shim[s - 2:s] = f[12:14]
    if fl & GTP:
        shim[30:32] = struct.pack(">H", L - 14)
    if fl & UDP:
        shim[24:26] = struct.pack(">H", L + s - 34)
    if fl & IP4:
        shim[2:4], shim[10:12] = struct.pack(">H", L + s - 14), b"\0\0"
        shim[10:12] = struct.pack(">H", csum(shim[:20]))
    v4 = f[12:14] == b"\x08\x00" and L >= 34 and f[14] >> 4 == 4 and f[14] & 15 >= 5
    if fl & TTL and (v4 or (f[12:14] == b"\x86\xdd" and L >= 54 and f[14] >> 4 == 6)):
        at = 8 if v4 else 7  # TTL at byte 22, hop limit at byte 21
        st |= nffacl.RW_TTL_DONE if inner[at] >= 2 else nffacl.RW_TTL_EXPIRED
        if inner[at] >= 2:
            if v4:  # RFC 1624 eq. 3: HC' = ~(~HC + ~m + m')
                hc, m = struct.unpack(">H", inner[10:12])[0], inner[8] << 8 | inner[9]
                x = (~hc & 0xFFFF) + (~m & 0xFFFF) + m - 0x100
                inner[10:12] = struct.pack(">H", csum(struct.pack(">I", x)))
            inner[at] -= 1
    head = (A["dmac"].tobytes() + A["smac"].tobytes() if fl & MACS else f[:12]) + (
        struct.pack(">H", int(A["ether_type"])) if s and A["ether_type"] else f[12:14])
    return head + bytes(shim) + bytes(inner), st


def pack(frames, desc, hop, adj, index, align):  # (bytes, descriptors, total, statuses) of the output batch
    out, od, status, raw, total = [], [], [], frames.tobytes(), 0
    for i in index:
        f, st = b"", 0
        if i < len(desc):
            o, ln, h = int(desc[i]) >> 16, int(desc[i]) & 0xFFFF, int(hop[i]) & 0xFFFFFF
            f, st = rewrite(raw[o:o + ln], adj[h]) if h < len(adj) else (raw[o:o + ln], 0)
        od.append(total << 16 | len(f))
        out.append(f + bytes(-len(f) % align))
        status.append(st)
        total += len(out[-1])
    out = np.frombuffer(b"".join(out), np.uint8)
    return out, np.array(od, np.uint64), len(out), np.array(status, np.uint8)


def launch(torch, router, b, adj, index, align, short=False, plain=False):  # guards behind d_out, out_desc, status
    want = pack(*b, adj, index, align)
    cap = want[2] // 2 // 16 * 16 if short else want[2]
    dev = [torch.from_numpy(a.view(t)).to("cuda") for a, t in
           ((b[0], np.uint8), (b[1], np.int64), (b[2], np.int32), (adj, np.uint8), (index, np.int32))]
    out = torch.full((want[2] + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out_desc = torch.full((len(index) + 1,), -1, dtype=torch.int64, device="cuda")
    out_bytes = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((len(index) + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    tail = (dev[4], len(index), out, cap, out_desc, out_bytes)
    if plain:
        router.gather_frames(dev[0], dev[1], len(b[1]), *tail, align)
    else:
        router.gather_encap_frames(dev[0], dev[1], len(b[1]), dev[2], dev[3] if len(adj) else None, len(adj), *tail,
                                   status, align)
    return want, cap, out, out_desc, out_bytes, status, dev


def check(want, cap, out, out_desc, out_bytes, status, _):
    got, gd, gs = out.cpu().numpy(), out_desc.cpu().numpy().view(np.uint64), status.cpu().numpy()
    assert int(out_bytes.cpu()[0]) == want[2] and gd[-1] == 0xFFFFFFFFFFFFFFFF and gs[-1] == 0xEE
    np.testing.assert_array_equal(gd[:-1], want[1])
    np.testing.assert_array_equal(gs[:-1], want[3])
    np.testing.assert_array_equal(got[:cap], want[0][:cap])  # headers, shifted data, clipped tails, zero pads
    assert (got[cap:] == 0xEE).all()  # nothing at or past out_cap, nor in the guard


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["identity", "reversed", "random"])
@pytest.mark.parametrize("align", [16, 64])
@pytest.mark.parametrize("m,short", [(0, False), (1, False), (63, False), (65, False), (T + 1, False),
                                     (2 * T + 37, False), (2 * T + 37, True)])
def test_gather_encap_matches_packing(torch, m, short, align, pattern):
    b, adj = batch(max(m, 1), m), table(RECORDS, 1)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, max(m, 1)) as r:
        res = launch(torch, r, b, adj, indices(pattern, len(b[1]), m, m + 1), align, short)
        torch.cuda.synchronize()
    if m >= 63:  # the batch exercises every outcome
        st = res[0][3]
        assert (st == 0).any() and all((st & bit).any() for bit in (1, 2, 4))
    check(*res)


@pytest.mark.gpu
@pytest.mark.parametrize("records", [[], [(0, 0, 0)] * len(RECORDS)])
def test_no_table_or_zero_records_is_the_plain_gather(torch, records):
    b, index = batch(T + 1, 5), indices("random", T + 1, T + 1, 6)
    b = (b[0], b[1], b[2] & 0xFFFFFF)
    adj = np.zeros(len(records), nffacl.ADJ_DTYPE)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, T + 1) as r:
        got, ref = launch(torch, r, b, adj, index, 64), launch(torch, r, b, adj[:0], index, 64, plain=True)
        torch.cuda.synchronize()
    check(*got)
    assert all(torch.equal(got[k], ref[k]) for k in (2, 3, 4))


def wire(i, rng):  # a well-formed frame with valid checksums and TTL 64: IPv4 / IPv6 x TCP / UDP / ICMP
    six, proto = i % 2 == 1, [(6, 17, 1), (6, 17, 58)][i % 2][i // 2 % 3]
    seg = bytearray(rng.integers(0, 256, {6: 20, 17: 8}.get(proto, 8) + 20 + i, dtype=np.uint8).tobytes())
    at = {6: 16, 17: 6}.get(proto, 2)  # the checksum field
    seg[at:at + 2] = b"\0\0"
    if proto == 6:
        seg[12] = 0x50
    if proto == 17:
        seg[4:6] = struct.pack(">H", len(seg))
    addr = rng.integers(1, 255, 32 if six else 8, dtype=np.uint8).tobytes()
    pseudo = addr + (struct.pack(">IHBB", len(seg), 0, 0, proto) if six else struct.pack(">BBH", 0, proto, len(seg)))
    seg[at:at + 2] = struct.pack(">H", csum((b"" if proto == 1 else pseudo) + bytes(seg)))
    if six:
        ip = struct.pack(">IHBB", 0x60000000, len(seg), proto, 64) + addr
    else:
        ip = bytearray(struct.pack(">BBHIBBH", 0x45, 0, 20 + len(seg), 0, 64, proto, 0) + addr)
        ip[10:12] = struct.pack(">H", csum(ip))
    return bytes(range(12)) + (b"\x86\xdd" if six else b"\x08\x00") + bytes(ip) + bytes(seg)


# (shim_len, flags, ether_type, shim): VLAN, QinQ, one and two MPLS labels, GRE over IPv4, GTP-U over IPv4, plain
CLOSING = [(4, INNER | TTL, 0x8100, b"\x00\x05"), (8, INNER, 0x88A8, b"\x00\x05\x81\x00\x00\x07"),
           (4, 0, 0x8847, b"\x00\x01\x01\x40"), (8, TTL, 0x8847, b"\x00\x01\x00\x40\x00\x01\x11\x40"),
           (24, IP4 | INNER, 0x0800, IP4H[:9] + b"\x2f" + IP4H[10:] + b"\0\0"),
           (36, IP4 | UDP | GTP | MACS | TTL, 0x0800, GTPU), (0, 0, 0, b"")]


@pytest.mark.gpu
def test_output_closes_with_keys_and_checksums(torch):
    rng = np.random.default_rng(29)
    adj = table([c[:3] for c in CLOSING], 2)
    for k, c in enumerate(CLOSING):
        adj["shim"][k, :len(c[3])] = np.frombuffer(c[3], np.uint8)
    n, buf, desc = 56, [], []
    for i in range(n):
        f = wire(i, rng)
        desc.append(sum(map(len, buf)) << 16 | len(f))
        buf.append(f + bytes(-len(f) % 16))
    hop = np.arange(n, dtype=np.int32) // 2 % len(CLOSING)  # every record meets both families
    s = adj["shim_len"][hop].astype(np.int64)
    frames = torch.from_numpy(np.frombuffer(b"".join(buf), np.uint8).copy()).to("cuda")
    d_desc, d_hop = torch.from_numpy(np.array(desc, np.int64)).to("cuda"), torch.from_numpy(hop).to("cuda")
    d_adj = torch.from_numpy(adj.view(np.uint8)).to("cuda")
    keys, keys2 = (torch.full((n, 4), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    key6, key6_2 = (torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    out = torch.zeros(frames.numel() + 128 * n, dtype=torch.uint8, device="cuda")
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    outer, inner = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, n) as r:
        nffacl.extract_keys_frames_device(frames, d_desc, n, keys, key6)
        r.gather_encap_frames(frames, d_desc, n, d_hop, d_adj, len(adj), torch.arange(n, dtype=torch.int32, device="cuda"),
                              n, out, out.numel(), out_desc, out_bytes, status)
        nffacl.extract_keys_encap_frames_device(out, out_desc, n, keys2, key6_2, ALL, offs)
        nffacl.checksum_frames_device(out, out_desc, n, outer, what=nffacl.CK_IP4)
        nffacl.checksum_frames_device(out, out_desc, n, inner, inner_off=offs)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(offs.cpu().numpy(), 14 + s)
    np.testing.assert_array_equal((out_desc & 0xFFFF).cpu().numpy(), (np.array(desc) & 0xFFFF) + s)
    assert torch.equal(keys2, keys) and torch.equal(key6_2, key6) and set((keys[:, 3] >> 8).cpu().tolist()) == {4, 6}
    ttl = (adj["flags"][hop] & TTL) != 0
    np.testing.assert_array_equal(status.cpu().numpy(), np.where(ttl, 3, 1))  # TTL 64: decremented where asked
    so, si = ((x >> 32).cpu().numpy() for x in (outer, inner))
    assert (so[s >= 24] & (nffacl.CK_IP4_DONE | nffacl.CK_IP4_BAD) == nffacl.CK_IP4_DONE).all()  # the GRE, GTP-U outers
    assert (si & (nffacl.CK_IP4_BAD | nffacl.CK_L4_BAD) == 0).all() and (si & nffacl.CK_L4_DONE != 0).all()
    assert (si[::2] & nffacl.CK_IP4_DONE != 0).all()  # the patched IPv4 header sums were looked at


@pytest.mark.gpu
def test_gather_encap_rejects_bad_arguments(torch):
    b, adj = batch(64, 3), table(RECORDS, 1)
    out = torch.full((1 << 18,), 0xEE, dtype=torch.uint8, device="cuda")
    od, ob = (torch.full((k,), -1, dtype=torch.int64, device="cuda") for k in (65, 1))
    st = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    frames, hop = torch.from_numpy(b[0]).to("cuda"), torch.from_numpy(b[2].view(np.int32)).to("cuda")
    d_adj = torch.from_numpy(adj.view(np.uint8)).to("cuda")
    good = [frames, torch.from_numpy(b[1].view(np.int64)).to("cuda"), 64, hop, d_adj, len(adj),
            torch.arange(64, dtype=torch.int32, device="cuda"), 64, out, 1 << 18, od, ob, st, 64]
    # (argument, value): bad align, bad out_cap, NULL / misaligned buffers, NULL hop, NULL adj, n_adj > 2^24, m > max_n
    bad = [(13, 24), (13, 8), (9, (1 << 18) + 8), (0, frames.data_ptr() + 4), (8, None), (8, out.data_ptr() + 8),
           (3, None), (3, hop.data_ptr() + 2), (4, None), (4, d_adj.data_ptr() + 8), (5, (1 << 24) + 1), (7, 65)]
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, 64) as r:
        for k, v in bad:
            with pytest.raises(nffacl.NFError) as e:
                r.gather_encap_frames(*good[:k], v, *good[k + 1:])
            assert e.value.status == nffacl.ERR_INVALID_ARG
        torch.cuda.synchronize()
    assert all((t.cpu().numpy() == v).all() for t, v in ((out, 0xEE), (st, 0xEE), (od, -1), (ob, -1)))  # no launch
