"""Classification from compact 5-tuple keys (nffacl_key, csrc/keys.hip):
extract_keys -> classify_keys against the CPU oracle on the slots the keys
came from, bit-exact, for every table kind; key semantics; host extraction
against the wire offsets; argument errors."""
import ctypes

import numpy as np
import pytest

import nffacl
from nffacl import synth
from oracle import oracle, rules_oracle as ro

N_MAX = (1 << 16) + 37
U = 2  # keys per lane per batch (csrc/keys.hpp kKeysU)
C5_20K = synth.RuleSpec(20000, sport=(0.0, 0.7, 0.3), dport=(0.5, 0.4, 0.1))
# name -> (rules text + generator, algo forced, algo expected, walk expected or None, slots or None)
CASES = {
    "fw_linear": ("fw", nffacl.ALGO_LINEAR, nffacl.ALGO_LINEAR, nffacl.WALK_LINEAR, None),
    "fw_indexed": ("fw", nffacl.ALGO_INDEXED, nffacl.ALGO_INDEXED, nffacl.WALK_INDEXED_LDS, None),
    "r300": (synth.RuleSpec(300), nffacl.ALGO_AUTO, nffacl.ALGO_INDEXED, nffacl.WALK_INDEXED_LDS, None),
    "r300_global": (synth.RuleSpec(300), nffacl.ALGO_AUTO, nffacl.ALGO_INDEXED, nffacl.WALK_INDEXED_GLOBAL, None),
    "r20k_hybrid": (C5_20K, nffacl.ALGO_HYBRID, nffacl.ALGO_HYBRID, None, None),
    "c5_fine6": (synth.SPECS["c5"], nffacl.ALGO_HYBRID, nffacl.ALGO_HYBRID, nffacl.WALK_FLAT_LDS_PIPELINED, 6),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def permit_bits(port):
    bits = np.zeros((len(port) + 63) // 64 * 64, np.uint64)
    bits[:len(port)] = port != 0
    return np.bitwise_or.reduce(bits.reshape(-1, 64) << np.arange(64, dtype=np.uint64), axis=1)


def run_keys(torch, eng, d_keys, d_key6, n_key6, n):
    """(ports, permit words) of classify_keys_device; outputs pre-filled with ones."""
    port = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    bits = torch.full(((n + 63) // 64 + 1,), -1, dtype=torch.int64, device="cuda")
    eng.classify_keys_device(d_keys, d_key6, n_key6, n, port, bits)
    torch.cuda.synchronize()
    return port.cpu().numpy().view(np.uint32)[:n], bits.cpu().numpy().view(np.uint64)[:(n + 63) // 64]


def via_keys(torch, eng, slots, stride, n, flags=0):
    d_slots = torch.from_numpy(slots).to("cuda")
    keys = torch.zeros((max(n, 1), 4), dtype=torch.int32, device="cuda")
    key6 = torch.zeros((max(n, 1), 8), dtype=torch.int32, device="cuda")
    nffacl.extract_keys_device(d_slots, stride, n, keys, key6, flags)
    return run_keys(torch, eng, keys, key6, n, n)


@pytest.fixture(scope="module", params=list(CASES))
def table(request, torch_cuda, golden):
    src, algo, want_algo, want_walk, want_slots = CASES[request.param]
    if src == "fw":
        text = (golden / "rules" / "firewall.conf").read_text()
        g = synth.firewall_rules(text)
    else:
        g = synth.gen_rules(src, synth.RULE_SEEDS["c5"])
        text = g.text
    a4, a6 = ro.parse_text_table(text.encode()).arrays()
    slots = synth.gen_slots(g, N_MAX, 71)  # the mix holds IHL 6-15, IPv6 and non-IP frames
    want = oracle.classify_slots(slots, 64, N_MAX, a4, a6, threads=16)
    with pytest.MonkeyPatch.context() as mp:
        if request.param == "r300_global":
            mp.setenv("NFFACL_TUNE_LDS", "0")  # read once, at engine creation
        eng = nffacl.Engine(nffacl.L3Rules.parse_text(text), algo=algo)
    with eng:
        k = eng.kernel_info()
        print(f"{request.param}: algo {eng.algo} walk {k.walk} slots {k.slots}")
        assert eng.algo == want_algo
        assert want_walk is None or k.walk == want_walk, k.walk
        assert want_slots is None or k.slots == want_slots, k.slots
        yield eng, slots, want, (a4, a6)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 64 * U - 1, 64 * U + 1, N_MAX])
def test_keys_equal_oracle(torch_cuda, table, n):
    eng, slots, want, _ = table
    p, b = via_keys(torch_cuda, eng, slots[:max(n, 1) * 64], 64, n)
    np.testing.assert_array_equal(p, want[:n])
    np.testing.assert_array_equal(b, permit_bits(want[:n]))  # zero bits past n in the last word


@pytest.mark.gpu
def test_keys_wide_slots_vlan(torch_cuda):
    """Stride 128, IHL 0..15, every other group of 16 frames 802.1Q-tagged,
    under NFFACL_PARSE_VLAN: ports past byte 63 are real bytes of the slot."""
    rng = np.random.default_rng(3)
    n = 4096 + 5
    buf = np.zeros((n, 128), np.uint8)
    for i in range(n):
        f = bytearray(rng.integers(0, 256, 128, dtype=np.uint8).tobytes())
        f[12:14] = b"\x08\x00"
        f[14] = 0x40 | (i % 16)
        f[23] = [6, 17, 1][i % 3]
        if (i // 16) % 2:
            f = f[:12] + bytearray(b"\x81\x00\x00\x05") + f[12:124]
        buf[i] = np.frombuffer(bytes(f), np.uint8)
    text = "\n".join(f"ANY ANY {p} {a}:{b} {c}:{d} {o}" for p, a, b, c, d, o in [
        ("TCP", 0, 30000, 0, 65535, 2), ("UDP", 20000, 65535, 100, 40000, 3), ("ANY", 0, 0, 0, 65535, 4),
        ("ANY", 0, 65535, 0, 0, 5), ("ANY", 1000, 50000, 1000, 50000, 6)]) + "\n"
    a4, a6 = ro.parse_text_table(text.encode()).arrays()
    slots = buf.reshape(-1)
    want = oracle.classify_slots(slots, 128, n, a4, a6, flags=nffacl.PARSE_VLAN)
    assert len(set(want.tolist())) > 3
    with nffacl.Engine(nffacl.L3Rules.parse_text(text)) as eng:
        p, _ = via_keys(torch_cuda, eng, slots, 128, n, nffacl.PARSE_VLAN)
    np.testing.assert_array_equal(p, want)


@pytest.mark.gpu
def test_key_semantics(torch_cuda, table):
    """Family 0, an unknown family and a family-6 index >= n_key6 give 0;
    their neighbours keep their verdicts.  The key6 buffer is larger than
    the n_key6 passed, so a missing bounds check reads a valid record."""
    torch = torch_cuda
    eng, slots, want, _ = table
    n = 4096
    keys = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    key6 = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    nffacl.extract_keys_device(torch.from_numpy(slots[:n * 64]).to("cuda"), 64, n, keys, key6)
    k = keys.cpu().numpy().view(nffacl.KEY_DTYPE).reshape(-1).copy()
    fam = (k["meta"] >> 8) & 0xFF
    hit4, hit6 = np.nonzero((fam == 4) & (want[:n] != 0))[0], np.nonzero(fam == 6)[0]
    n_key6 = int(hit6[len(hit6) // 2])  # IPv6 packets at or past this index fall out of range
    exp = want[:n].copy()
    exp[hit6[hit6 >= n_key6]] = 0
    k["meta"][hit4[0]] &= 0xFF  # family 0
    k["meta"][hit4[1]] = (k["meta"][hit4[1]] & 0xFF) | 5 << 8  # unknown family
    k["meta"][hit4[2]] |= 1 << 16  # family 4 with a reserved bit set: unknown too
    exp[hit4[:3]] = 0
    assert (exp != 0).sum() > 10
    p, b = run_keys(torch, eng, torch.from_numpy(k.view(np.uint32)).to("cuda"), key6, n_key6, n)
    np.testing.assert_array_equal(p, exp)
    np.testing.assert_array_equal(b, permit_bits(exp))


def host_keys(slots, n, stride=64, flags=0):
    buf = np.ascontiguousarray(slots[:n * stride])
    ptrs = np.uint64(buf.ctypes.data) + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    return nffacl.extract_keys_host(ptrs, np.full(n, stride, np.uint32), flags)


def test_extract_keys_host_wire_offsets():
    """IHL-5 untagged IPv4 and IPv6 frames: every key field is the bytes at its wire offset."""
    g = synth.gen_rules(synth.RuleSpec(300), 5)
    n = 4096
    s = synth.gen_slots(g, n, 9).reshape(n, 64)
    keys, key6 = host_keys(s.reshape(-1), n)
    et = s[:, 12].astype(np.uint32) << 8 | s[:, 13]
    v4, v6 = (et == 0x0800) & (s[:, 14] == 0x45), et == 0x86DD
    assert v4.sum() > 1000 and v6.sum() > 100 and len(key6) == v6.sum()
    w = s.astype(np.uint32)

    def le32(o):
        return w[:, o] | w[:, o + 1] << 8 | w[:, o + 2] << 16 | w[:, o + 3] << 24

    def ports(o):  # sport | dport << 16, host-order numbers
        return (w[:, o] << 8 | w[:, o + 1]) | (w[:, o + 2] << 8 | w[:, o + 3]) << 16
    np.testing.assert_array_equal(keys["a"][v4], le32(26)[v4])
    np.testing.assert_array_equal(keys["b"][v4], le32(30)[v4])
    np.testing.assert_array_equal(keys["ports"][v4], ports(34)[v4])
    np.testing.assert_array_equal(keys["meta"][v4], s[v4, 23].astype(np.uint32) | 4 << 8)
    np.testing.assert_array_equal(keys["a"][v6], np.arange(v6.sum()))  # dense, arrival order
    np.testing.assert_array_equal(keys["ports"][v6], ports(54)[v6])
    np.testing.assert_array_equal(keys["meta"][v6], s[v6, 20].astype(np.uint32) | 6 << 8)
    np.testing.assert_array_equal(key6["src"], s[v6, 22:38])
    np.testing.assert_array_equal(key6["dst"], s[v6, 38:54])
    assert (keys[~(et == 0x0800) & ~v6].view(np.uint32) == 0).all()


@pytest.mark.gpu
def test_host_keys_and_classify_keys_host(torch_cuda, table):
    """Host-extracted keys give the device path's verdicts (their key6 indices
    differ), through classify_keys_device and through classify_keys_host."""
    torch = torch_cuda
    eng, slots, want, _ = table
    keys, key6 = host_keys(slots, N_MAX)
    p, _ = run_keys(torch, eng, torch.from_numpy(keys.view(np.uint32)).to("cuda"),
                    torch.from_numpy(key6.view(np.uint8)).to("cuda"), len(key6), N_MAX)
    np.testing.assert_array_equal(p, want)
    port, perm = eng.classify_keys_host(keys, key6)
    np.testing.assert_array_equal(port, want)
    np.testing.assert_array_equal(perm, want != 0)


def test_key_argument_errors():
    """Checked before any device work, so no GPU is needed."""
    lib = ctypes.CDLL(str(nffacl.LIB_PATH))
    buf = np.zeros(64, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16  # a 16-byte aligned address inside buf
    eng, bad = ctypes.c_void_p(1), nffacl.ERR_INVALID_ARG  # (never dereferenced: the checks come first)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    dev = lib.nffacl_classify_keys_device
    dev.argtypes = [vp, vp, vp, u32, u64, vp, vp, vp]
    assert dev(eng, None, None, 0, 1, a, None, None) == bad       # NULL keys, n > 0
    assert dev(eng, a, None, 0, 1, None, None, None) == bad       # both outputs NULL
    assert dev(eng, a + 4, None, 0, 1, a, None, None) == bad      # misaligned keys
    host = lib.nffacl_classify_keys_host
    host.argtypes = [vp, vp, vp, u32, u64, vp, vp]
    assert host(eng, None, None, 0, 1, a, None) == bad
    assert host(eng, a, None, 0, 1, None, None) == bad
    assert host(eng, a + 4, None, 0, 1, a, None) == bad
    frame = np.zeros(64, np.uint8)
    frame[12:14] = (0x86, 0xDD)
    ptrs = np.full(2, frame.ctypes.data, np.uint64)
    with pytest.raises(nffacl.NFError) as e:  # two IPv6 frames, room for one record
        nffacl.extract_keys_host(ptrs, np.full(2, 64, np.uint32), key6_cap=1)
    assert e.value.status == bad
