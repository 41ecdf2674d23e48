"""Keys of encapsulated packed frames (csrc/keys_encap.hip) against the plain parse of the decapsulated frame
(extract_keys_host), their verdicts against the oracle on the decapsulated batch.  Every comparison is exact."""
import struct

import numpy as np
import pytest

import nffacl
from oracle import oracle, rules_oracle as ro

N = 4103
V, M, G, T = nffacl.ENCAP_VLAN, nffacl.ENCAP_MPLS, nffacl.ENCAP_GRE, nffacl.ENCAP_GTPU
ALL = V | M | G | T
TEXT = "\n".join(f"ANY ANY {p} {a}:{b} {c}:{d} {o}" for p, a, b, c, d, o in [  # the table of tests/test_keys_frames.py
    ("TCP", 0, 30000, 0, 65535, 2), ("UDP", 20000, 65535, 100, 40000, 3), ("ANY", 0, 0, 0, 65535, 4),
    ("ANY", 0, 65535, 0, 0, 5), ("ANY", 1000, 50000, 1000, 50000, 6)]) + "\n"
# a layer: ("tag", TPID) | ("mpls", labels, last label has S) | ("gre", outer family, flag byte)
#          | ("gtp", outer family, outer IHL, flag byte, extension lengths in 4-octet units)
KINDS = [
    [], [("tag", 0x8100)], [("tag", 0x88A8), ("tag", 0x8100)],
    [("mpls", 1, 1)], [("mpls", 3, 1)], [("mpls", 8, 1)],
    [("gre", 4, 0x00)], [("gre", 4, 0xB0)], [("gre", 6, 0x00)],
    [("gtp", 4, 5, 0x30, ())], [("gtp", 4, 5, 0x32, ())], [("gtp", 4, 5, 0x34, (1,))], [("gtp", 4, 5, 0x36, (1, 2))],
    [("gtp", 4, 7, 0x30, ())], [("gtp", 6, 5, 0x30, ())],
    [("tag", 0x8100), ("mpls", 2, 1)], [("tag", 0x8100), ("gtp", 4, 5, 0x30, ())], [("mpls", 1, 1), ("gre", 4, 0x20)],
    [("mpls", 6, 1), ("gtp", 4, 15, 0x34, (10,))],  # cursor 158: the inner window runs past the staged 192 bytes
    [("gtp", 4, 5, 0x34, (25, 25))],                # the extension chain itself runs past them
    [("tag", 0x88A8), ("tag", 0x8100), ("mpls", 1, 1), ("gre", 6, 0x80)],
    # malformed: 9 labels, no bottom of stack before the frame ends, an extension of length 0, 5 extensions
    [("mpls", 9, 1)], [("mpls", 5, 0)], [("gtp", 4, 5, 0x34, (0,))], [("gtp", 4, 5, 0x34, (1, 1, 1, 1, 1))],
]
ET = {4: 0x0800, 6: 0x86DD}


def outer_ip(fam, proto, ihl=5):
    if fam == 6:
        return bytes([0x60, 0, 0, 0, 0, 0, proto, 64]) + bytes(range(32))
    return bytes([0x40 | ihl, 0, 0, 0, 0, 0, 0, 0, 64, proto, 0, 0, 10, 1, 2, 3, 10, 4, 5, 6]) + bytes(4 * (ihl - 5))


def wrap(layers, et):
    """(outer EtherType, shim bytes, per layer (flag, size, its own EtherType, bytes from its start that identify
    it, malformed)) of `layers` around a payload of EtherType `et`, built inside out."""
    shim, info = b"", []
    for kind, *a in reversed(layers):
        if kind == "tag":
            part, et, row = struct.pack(">HH", 5, et), a[0], (V, 0, False)
        elif kind == "mpls":
            part = b"".join(struct.pack(">I", (16 + i) << 12 | (a[1] and i == a[0] - 1) << 8 | 64) for i in range(a[0]))
            et, row = 0x8847, (M, 0, a[0] > 8 or not a[1])
        elif kind == "gre":
            part = outer_ip(a[0], 47) + bytes([a[1], 0]) + struct.pack(">H", et) + bytes(4 * bin(a[1] & 0xB0).count("1"))
            et, row = ET[a[0]], (G, 10 if a[0] == 4 else 7, False)
        else:
            fam, ihl, fl, exts = a
            ip = outer_ip(fam, 17, ihl)
            part = ip + struct.pack(">HHHH", 1234, 2152, 0, 0) + bytes([fl, 255, 0, 0, 0, 0, 0, 9])
            if fl & 7:
                part += bytes([0, 1, 0, 0x85 if exts else 0])
            for j, ln in enumerate(exts):
                part += bytes([ln]) + bytes(max(4 * ln, 4) - 2) + bytes([0x85 if j + 1 < len(exts) else 0])
            et, row = ET[fam], (T, len(ip) + 10, 0 in exts or len(exts) > 4)
        shim, info = part + shim, [(row[0], len(part), et, row[1], row[2])] + info
    return et, shim, info


@pytest.fixture(scope="module")
def batch():
    """Inner frames as tests/test_keys_frames.py builds them, frame i wrapped in KINDS[i % len(KINDS)]; packed
    wire frames with descriptors, and per frame (whole wire frame, inner EtherType, layer info, length)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    rng = np.random.default_rng(17)
    buf, desc, meta, off = [], [], [], 0
    for i in range(N):
        six = i % 8 == 5
        f = bytearray(rng.integers(0, 256, 128, dtype=np.uint8).tobytes())
        f[12:14] = struct.pack(">H", ET[6 if six else 4])
        f[14] = (0x60 if six else 0x40) | (i % 16)
        f[20 if six else 23] = [6, 17, 1][i % 3]
        et, shim, info = wrap(KINDS[i % len(KINDS)], ET[6 if six else 4])
        wire = bytes(f[:12]) + struct.pack(">H", et) + shim + bytes(f[14:])
        if KINDS[i % len(KINDS)] == [("mpls", 5, 0)]:
            wire = wire[:14 + len(shim)]  # the frame ends before any bottom of stack
        t = len(shim)  # full, a cut inside the inner L4, inside the inner L3, inside the shims, and 40
        ln = min([t + 128, t + 36, t + 28, t + 13, 40][(i // len(KINDS)) % 5], len(wire))
        buf.append(wire[:ln] + bytes(-ln % 64))  # 64-byte rooms
        desc.append(off << 16 | ln)
        meta.append((wire, ET[6 if six else 4], info, ln))
        off += len(buf[-1])
    frames, desc = np.frombuffer(b"".join(buf), np.uint8).copy(), np.array(desc, np.uint64)
    dev = torch.from_numpy(frames).to("cuda"), torch.from_numpy(desc.view(np.int64)).to("cuda")
    return torch, frames, desc, dev, meta


def decapsulate(meta, encap):
    """Packed decapsulated frames, their descriptors and cursors: the leading layers enabled in `encap` stripped,
    stopping at the first that is disabled or whose identifying bytes the frame's length cuts off (bytes past the
    length read as 0, so such a frame does not carry the layer); malformed frames become 14 zero bytes."""
    buf, desc, cursor, off = [], [], [], 0
    for wire, et, info, ln in meta:
        strip, bad = 0, False
        for flag, size, own, ident, malformed in info:
            if not flag & encap or 14 + strip + ident > ln:
                et = own
                break
            strip, bad = strip + size, bad or malformed
        bad = bad or (strip > 0 and 14 + strip >= ln)
        plain = bytes(14) if bad else (wire[:12] + struct.pack(">H", et) + wire[14 + strip:])[:ln - strip]
        cursor.append(0xFFFF if bad else 14 + strip)
        buf.append(plain + bytes(-len(plain) % 64))
        desc.append(off << 16 | len(plain))
        off += len(buf[-1])
    return np.frombuffer(b"".join(buf), np.uint8).copy(), np.array(desc, np.uint64), np.array(cursor, np.uint16)


def run(batch, n, encap, inner_off=True):
    torch, dev = batch[0], batch[3]
    keys = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    key6 = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    offs = torch.full((n,), 7, dtype=torch.int16, device="cuda") if inner_off else None
    nffacl.extract_keys_encap_frames_device(dev[0], dev[1], n, keys, key6, encap, offs)
    return keys, key6, offs


def check_keys(keys, key6, plain, pdesc):
    """keys / key6 (device) are extract_keys_host's of the packed frames plain / pdesc, as test_keys_from_frames."""
    got, got6 = (t.cpu().numpy().view(d).reshape(-1) for t, d in ((keys, nffacl.KEY_DTYPE), (key6, nffacl.KEY6_DTYPE)))
    want, want6 = nffacl.extract_keys_host(np.uint64(plain.ctypes.data) + (pdesc >> np.uint64(16)),
                                           (pdesc & np.uint64(0xFFFF)).astype(np.uint32), 0)
    six = (want["meta"] >> 8) == 6
    for field in ("b", "ports", "meta"):
        np.testing.assert_array_equal(got[field], want[field])
    np.testing.assert_array_equal(got["a"][~six], want["a"][~six])
    np.testing.assert_array_equal(got["a"][six], np.nonzero(six)[0])  # an IPv6 record lies at its frame's index
    np.testing.assert_array_equal(got6[got["a"][six]], want6[want["a"][six]])


@pytest.mark.gpu
@pytest.mark.parametrize("encap", [ALL, V, M, G, T, V | T, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, N])
def test_keys_from_encapsulated_frames(batch, n, encap):
    torch, frames, desc = batch[0], batch[1], batch[2][:n]
    plain, pdesc, cursor = decapsulate(batch[4][:n], encap)
    keys, key6, offs = run(batch, n, encap)
    torch.cuda.synchronize()
    check_keys(keys, key6, plain, pdesc)
    np.testing.assert_array_equal(offs.cpu().numpy().view(np.uint16), cursor)
    if encap == 0:  # the plain call
        k0, k6 = torch.full_like(keys, -1), torch.zeros_like(key6)
        nffacl.extract_keys_frames_device(batch[3][0], batch[3][1], n, k0, k6)
        assert torch.equal(k0, keys) and torch.equal(k6, key6) and (cursor == 14).all()
    if encap == ALL and n == N:  # the inner keys' verdicts are the oracle's on the decapsulated frames
        a4, a6 = ro.parse_text_table(TEXT.encode()).arrays()
        port = torch.zeros(n, dtype=torch.int32, device="cuda")
        with nffacl.Engine(nffacl.L3Rules.parse_text(TEXT)) as eng:
            eng.classify_keys_device(keys, key6, n, n, port)
            torch.cuda.synchronize()
        verdicts = oracle.classify_frames(plain, pdesc, a4, a6, flags=0)
        assert len(set(verdicts.tolist())) > 3 and (cursor == 0xFFFF).any()
        assert (verdicts[cursor == 0xFFFF] == 0).all()
        np.testing.assert_array_equal(port.cpu().numpy().view(np.uint32), verdicts)


@pytest.mark.gpu
def test_no_inner_off_and_invalid_arguments(batch):
    torch, dev = batch[0], batch[3]
    plain, pdesc, _ = decapsulate(batch[4][:200], ALL)
    keys, key6, _ = run(batch, 200, ALL, inner_off=False)
    torch.cuda.synchronize()
    check_keys(keys, key6, plain, pdesc)
    k, k6 = keys.data_ptr(), key6.data_ptr()
    for frames, d, n, encap, kk, kk6, offs in [
            (dev[0], dev[1], 200, 16, k, k6, None), (dev[0], dev[1], 200, ALL, None, k6, None),
            (None, dev[1], 200, ALL, k, k6, None), (dev[0], None, 200, ALL, k, k6, None),
            (dev[0], dev[1], 200, ALL, k, None, None), (dev[0], dev[1], 200, ALL, k + 8, k6, None),
            (dev[0].data_ptr() + 4, dev[1], 200, ALL, k, k6, None), (dev[0], dev[1], 200, ALL, k, k6 + 4, None),
            (dev[0], dev[1], 200, ALL, k, k6, k + 1), (dev[0], dev[1], 1 << 32, ALL, k, k6, None)]:
        with pytest.raises(nffacl.NFError) as e:
            nffacl.extract_keys_encap_frames_device(frames, d, n, kk, kk6, encap, offs)
        assert e.value.status == nffacl.ERR_INVALID_ARG
