"""Decapsulating packed-frame gather (csrc/route_decap.hip), exact against a numpy packing written from nffacl.h."""
import struct

import numpy as np
import pytest

import nffacl

T = (1 << 20) // nffacl.route_frames_plan(1 << 20)[0]  # frames per tile
STRIPS = [0, 4, 8, 12, 16, 20, 36, 52, 144]            # every s % 16, s >= 16, a strip past the first 128 bytes
ALL = nffacl.ENCAP_VLAN | nffacl.ENCAP_MPLS | nffacl.ENCAP_GRE | nffacl.ENCAP_GTPU


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def batch(n, seed, plain=False):
    """n random frames in 16-byte rooms (0xA5 past each length, the buffer sized exactly), descriptors, cursors
    (14 + a strip of STRIPS; about 10 % ones the rule must ignore) and keys with families of {0, 4, 6}."""
    rng = np.random.default_rng(seed)
    s = rng.choice(STRIPS, n)
    ln = np.where(rng.random(n) < 0.3, rng.choice([15, 16, 17, 31, 32, 33], n), rng.integers(15, 1519, n)) + s
    odd = np.stack([np.full(n, 14), np.full(n, 0xFFFF), np.full(n, 13), np.full(n, 15), ln, ln + 4])
    cur = np.where(rng.random(n) < 0.1, odd[rng.integers(0, 6, n), np.arange(n)], 14 + s)
    room = (ln + 15) // 16 * 16
    off = np.cumsum(room) - room
    frames = rng.integers(0, 256, int(room.sum()), dtype=np.uint8)
    frames[np.arange(len(frames)) - np.repeat(off, room) >= np.repeat(ln, room)] = 0xA5
    keys = np.zeros(n, nffacl.KEY_DTYPE)
    keys["meta"] = rng.choice([0, 4, 6], n) << 8 | 6
    cur = np.full(n, 14) if plain else cur
    return frames, off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64), cur.astype(np.uint16), keys


def indices(pattern, n, m, seed):
    if pattern == "random":  # repeats, about 1 % past the batch
        rng = np.random.default_rng(seed)
        idx = rng.integers(0, n, m)
        bad = rng.random(m) < 0.01
        idx[bad] = rng.choice([n, n + 1, 0xFFFFFFFF], int(bad.sum()))
        return idx.astype(np.uint32)
    return np.arange(m, dtype=np.uint32)[::-1 if pattern == "reversed" else 1].copy()


def pack(frames, desc, cur, keys, index, align):  # (bytes, descriptors, total) of the output batch, as nffacl.h defines it
    ok, i = index < len(desc), np.minimum(index, len(desc) - 1)
    d, c = np.where(ok, desc[i], 0).astype(np.int64), np.where(ok, cur[i], 0).astype(np.int64)
    ln, src = d & 0xFFFF, d >> 16
    s = np.where((c > 14) & (c < ln) & ((c - 14) % 4 == 0), c - 14, 0)
    ln = ln - s
    room = (ln + align - 1) // align * align
    off = np.cumsum(room) - room
    out = np.zeros(int(room.sum()), np.uint8)
    within = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    # bytes [12, 14) <- source [c - 2, c), bytes [14, L') <- source [c, L); then the EtherType of families 4 and 6
    out[np.repeat(off, ln) + within] = frames[np.repeat(src, ln) + within + np.where(within >= 12, np.repeat(s, ln), 0)]
    fam = keys["meta"][i].astype(np.int64) >> 8 & 0xFF
    for family, et in ((4, (0x08, 0x00)), (6, (0x86, 0xDD))):
        at = off[(s > 0) & (fam == family)]
        out[at + 12], out[at + 13] = et
    return out, off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64), len(out)


def launch(torch, router, b, index, align, short=False, plain=False):  # guards behind d_out and out_desc
    want = pack(*b, index, align)
    cap = want[2] // 2 // 16 * 16 if short else want[2]
    dev = [torch.from_numpy(a.view(t)).to("cuda") for a, t in
           ((b[0], np.uint8), (b[1], np.int64), (b[2], np.int16), (b[3], np.uint8), (index, np.int32))]
    out = torch.full((want[2] + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out_desc = torch.full((len(index) + 1,), -1, dtype=torch.int64, device="cuda")
    out_bytes = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    tail = (dev[4], len(index), out, cap, out_desc, out_bytes, align)
    if plain:
        router.gather_frames(dev[0], dev[1], len(b[1]), *tail)
    else:
        router.gather_decap_frames(dev[0], dev[1], len(b[1]), dev[2], dev[3], *tail)
    return want, cap, out, out_desc, out_bytes, dev


def check(want, cap, out, out_desc, out_bytes, _):
    got, gd = out.cpu().numpy(), out_desc.cpu().numpy().view(np.uint64)
    assert int(out_bytes.cpu()[0]) == want[2] and gd[-1] == 0xFFFFFFFFFFFFFFFF
    np.testing.assert_array_equal(gd[:-1], want[1])
    np.testing.assert_array_equal(got[:cap], want[0][:cap])  # data, shifted data, clipped tails, zero pads
    assert (got[cap:] == 0xEE).all()  # nothing at or past out_cap, nor in the guard


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["identity", "reversed", "random"])
@pytest.mark.parametrize("align", [16, 64])
@pytest.mark.parametrize("m,short", [(0, False), (1, False), (63, False), (65, False), (T + 1, False),
                                     (2 * T + 37, False), (2 * T + 37, True)])
def test_gather_decap_matches_packing(torch, m, short, align, pattern):
    b = batch(max(m, 1), m)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, max(m, 1)) as r:
        res = launch(torch, r, b, indices(pattern, len(b[1]), m, m + 1), align, short)
        torch.cuda.synchronize()
    check(*res)


@pytest.mark.gpu
def test_cursor_14_is_the_plain_gather(torch):
    b = batch(T + 1, 5, plain=True)
    index = indices("random", T + 1, T + 1, 6)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, T + 1) as r:
        got, ref = launch(torch, r, b, index, 64), launch(torch, r, b, index, 64, plain=True)
        torch.cuda.synchronize()
    check(*got)
    assert all(torch.equal(got[k], ref[k]) for k in (2, 3, 4))


IP4 = bytes([0x45, 0, 0, 0, 0, 0, 0, 0, 64, 17, 0, 0, 10, 1, 2, 3, 10, 4, 5, 6])  # protocol UDP; byte 9 = 47 for GRE
GTPU = IP4 + struct.pack(">HHHH", 1234, 2152, 0, 0) + bytes([0x30, 255, 0, 0, 0, 0, 0, 9])  # byte 28: the GTP flags
# (outer EtherType or None for the inner one, shim bytes); b"<>" stands for the inner EtherType
SHIMS = [(None, b""), (0x8100, b"\x00\x05<>"), (0x88A8, b"\x00\x05\x81\x00\x00\x07<>"),
         (0x8847, b"\x00\x01\x00\x40\x00\x01\x10\x40\x00\x01\x21\x40"),
         (0x0800, IP4[:9] + b"\x2f" + IP4[10:] + b"\x00\x00<>"),
         (0x86DD, bytes([0x60, 0, 0, 0, 0, 0, 47, 64]) + bytes(range(32)) + b"\x20\x00<>\x00\x00\x00\x07"),
         (0x0800, GTPU), (0x0800, GTPU[:28] + b"\x34" + GTPU[29:] + b"\x00\x00\x00\x85" + b"\x01\x00\x00\x00"),
         (0x8100, b"\x00\x05\x08\x00" + GTPU)]


@pytest.mark.gpu
def test_plain_keys_of_the_output_are_the_encap_keys(torch):
    rng = np.random.default_rng(23)
    buf, desc, shim_len = [], [], []
    for i in range(54):  # every shim around IPv4 and IPv6 with TCP, UDP and ICMP
        six, (outer, shim) = i % 2 == 1, SHIMS[i % len(SHIMS)]
        et = struct.pack(">H", 0x86DD if six else 0x0800)
        f = bytearray(rng.integers(0, 256, 100 + i, dtype=np.uint8).tobytes())
        f[14], f[20 if six else 23] = (0x60 if six else 0x45), [6, 17, 1][i // 2 % 3]
        wire = bytes(f[:12]) + (struct.pack(">H", outer) if outer else et) + shim.replace(b"<>", et) + bytes(f[14:])
        desc.append(sum(map(len, buf)) << 16 | len(wire))
        buf.append(wire + bytes(-len(wire) % 16))
        shim_len.append(len(shim))
    n, frames = len(desc), torch.from_numpy(np.frombuffer(b"".join(buf), np.uint8).copy()).to("cuda")
    d_desc = torch.from_numpy(np.array(desc, np.int64)).to("cuda")
    keys, keys2 = (torch.full((n, 4), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    key6, key6_2 = (torch.zeros((n, 8), dtype=torch.int32, device="cuda") for _ in range(2))
    offs = torch.zeros(n, dtype=torch.int16, device="cuda")
    out = torch.zeros(frames.numel() + 64 * n, dtype=torch.uint8, device="cuda")
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, n) as r:
        nffacl.extract_keys_encap_frames_device(frames, d_desc, n, keys, key6, ALL, offs)
        r.gather_decap_frames(frames, d_desc, n, offs, keys, torch.arange(n, dtype=torch.int32, device="cuda"), n,
                              out, out.numel(), out_desc, out_bytes)
        nffacl.extract_keys_frames_device(out, out_desc, n, keys2, key6_2)
        torch.cuda.synchronize()
    np.testing.assert_array_equal(offs.cpu().numpy(), 14 + np.array(shim_len))  # none is malformed
    np.testing.assert_array_equal((out_desc & 0xFFFF).cpu().numpy(), (np.array(desc) & 0xFFFF) - np.array(shim_len))
    assert set((keys[:, 3] >> 8).cpu().tolist()) == {4, 6}
    assert torch.equal(keys2, keys) and torch.equal(key6_2, key6)


@pytest.mark.gpu
def test_gather_decap_rejects_bad_arguments(torch):
    b = batch(64, 3)
    out = torch.full((1 << 17,), 0xEE, dtype=torch.uint8, device="cuda")
    od, ob = (torch.full((k,), -1, dtype=torch.int64, device="cuda") for k in (65, 1))
    keys = torch.from_numpy(b[3].view(np.uint8)).to("cuda")
    good = [torch.from_numpy(b[0]).to("cuda"), torch.from_numpy(b[1].view(np.int64)).to("cuda"), 64,
            torch.from_numpy(b[2].view(np.int16)).to("cuda"), keys, torch.arange(64, dtype=torch.int32, device="cuda"),
            64, out, 1 << 17, od, ob, 64]
    # (argument, value): NULL inner_off, NULL keys, misaligned keys, m > max_n, bad align
    bad = [(3, None), (4, None), (4, keys.data_ptr() + 8), (6, 65), (11, 24), (11, 8)]
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, 64) as r:
        for k, v in bad:
            with pytest.raises(nffacl.NFError) as e:
                r.gather_decap_frames(*good[:k], v, *good[k + 1:])
            assert e.value.status == nffacl.ERR_INVALID_ARG
        torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xEE).all() and (od.cpu().numpy() == -1).all() and int(ob.cpu()[0]) == -1  # no launch
