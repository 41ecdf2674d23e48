"""Longest-prefix-match next hops (csrc/lpm.cpp, csrc/lpm.hip), exact against a brute-force longest match."""
import json
from pathlib import Path

import numpy as np
import pytest

import nffacl
from nffacl import LPM_FORCE_GLOBAL, LPM_FORCE_LDS, LPM_SWAP_BYTES

KATS = json.loads((Path(__file__).parent / "golden" / "lpm_kats.json").read_text())
U32 = 0xFFFFFFFF
MISS = 7      # also a legal hop of the edge table: only the bitmap tells them apart
SENT = -0x5A5A5A5B  # guard pattern after both outputs


def mask(d):
    return (U32 << (32 - d)) & U32


def reference(rules, addr):
    """(hit, hop) per address: the deepest rule {(masked ip, depth): hop} whose masked value equals the masked address."""
    best, hop = np.zeros(len(addr), np.int64), np.zeros(len(addr), np.uint32)
    for (ip, d), h in rules.items():
        m = ((addr & np.uint32(mask(d))) == ip) & (d > best)
        best[m], hop[m] = d, h
    return best > 0, hop


def table(rules, max_rules=1000, tbl8=1 << 16):
    lpm = nffacl.CreateLPM("lpm", 0, max_rules, tbl8)
    for (ip, d), h in rules.items():
        assert lpm.Add(ip, d, h) == 0
    return lpm


def edge_rules():
    """Every depth 1..32; a nested chain across both level edges; a /16 leaf beside a /16 with a group; hops 0, 2^24 - 1."""
    rng, rules = np.random.default_rng(15), {}
    for d in range(1, 33):  # depths below 8 keep to the top of the space: the lower half stays partly uncovered
        for ip in ([mask(d)] if d < 8 else rng.integers(0, 1 << 32, 11)):
            rules[(int(ip) & mask(d), d)] = int(rng.integers(0, 1 << 24))
    for d, h in zip((8, 14, 15, 16, 17, 23, 24, 25, 31, 32), (1, 2, 3, 0, 5, 6, MISS, 8, 9, 0xFFFFFF)):
        rules[(0x0A141E29 & mask(d), d)] = h
    rules.update({(0x55550000, 16): 40, (0x55560000, 16): 41, (0x55560100, 24): 42})
    return rules


def edge_addresses(rules, n):
    """Each rule's first and last address and the two just outside, uncovered ones, random fill; shuffled."""
    rng = np.random.default_rng(16)
    a = [x & U32 for (ip, d) in rules for x in (ip, ip | (U32 >> d), ip - 1, (ip | (U32 >> d)) + 1)]
    a += [0x00000000, 0x00FFFFFF, 0x30000001, 0x55570000, 0x5554FFFF]
    a = np.concatenate([np.array(a, np.uint32), rng.integers(0, 1 << 32, n - len(a), dtype=np.uint32)])
    return rng.permutation(a)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


@pytest.fixture(scope="module")
def edge(torch):
    rules = edge_rules()
    assert 250 <= len(rules) <= 350 and {d for _, d in rules} == set(range(1, 33))
    lpm = table(rules)
    lpm.commit()
    addr = edge_addresses(rules, 3 * 4096 + 37)
    hit = reference(rules, addr)[0]
    assert hit.any() and not hit.all()
    yield lpm, rules, addr
    lpm.Free()


def check(torch, lpm, rules, addr, keys=False, flags=0, miss=MISS, stream=None):
    """One lookup of addr (dense, or as the b of keys with other families mixed in), exact: next hops, every bitmap
    word, guards behind both outputs.  Returns a closure that compares after the caller synchronises."""
    n, words = len(addr), (len(addr) + 63) // 64
    look = addr.byteswap() if flags & LPM_SWAP_BYTES else addr
    hit, hop = reference(rules, look)
    if keys:
        k = np.zeros(n, nffacl.KEY_DTYPE)
        fam = np.where(np.arange(n) % 5 == 1, 0, np.where(np.arange(n) % 7 == 2, 6, 4)).astype(np.uint32)
        k["a"], k["b"], k["ports"], k["meta"] = ~addr, addr, 0x00500050, fam << 8 | 6
        hit = hit & (fam == 4)
        src = torch.from_numpy(k.view(np.uint8)).cuda()
    else:
        src = torch.from_numpy(addr.view(np.int32)).cuda()
    nxt = torch.full((n + 8,), SENT, dtype=torch.int32, device="cuda")
    bits = torch.full((words + 2,), SENT, dtype=torch.int64, device="cuda")
    call = lpm.lookup_keys_device if keys else lpm.lookup_device
    call(src, n, nxt, bits, flags=flags, miss_value=miss, stream=stream)

    def compare():
        got, gb = nxt.cpu().numpy(), bits.cpu().numpy()
        want = np.where(hit, hop, np.uint32(miss))
        assert (got[:n].view(np.uint32) == want).all(), np.flatnonzero(got[:n].view(np.uint32) != want)[:8]
        pad = np.zeros(words * 64, np.uint8)
        pad[:n] = hit
        assert (gb[:words].view(np.uint64) == np.packbits(pad, bitorder="little").view("<u8")).all()
        assert (got[n:] == SENT).all() and (gb[words:] == SENT).all()
    return compare


def play(steps, lookup):
    """The KAT sequence on a fresh table; lookup(lpm, dirty, ip) -> (hit, hop)."""
    lpm, dirty = nffacl.CreateLPM("lpm", 0, KATS["max_rules"], KATS["number_tbl8"]), True
    for s in steps:
        ip = int(s["ip"], 16)
        if s["op"] == "lookup":
            hit, hop = lookup(lpm, dirty, ip)
            assert (hit, hop if hit else 0) == (s["hit"], s["hop"]), s
            dirty = False
        else:
            st = lpm.Add(ip, s["depth"], s["hop"]) if s["op"] == "add" else lpm.Delete(ip, s["depth"])
            assert (st == 0) == s["ok"] and st in (0, nffacl.ERR_INVALID_ARG), s
            dirty = True
    assert lpm.count() == KATS["rules_left"]
    lpm.Free()


def walk(blob, a):
    """One address through the table nffacl.h describes."""
    H, off_l0, off_hops, off_l1, off_l2 = (int(x) for x in blob[[1, 4, 5, 6, 7]])
    e = int(blob[off_l0:off_hops].view(np.uint16)[a >> 16])
    w = int(blob[off_hops + e]) if e <= H else int(blob[off_l1 + 256 * (e - H - 1) + (a >> 8 & 0xFF)])
    if w & 1 << 30:
        w = int(blob[off_l2 + 256 * (w & 0xFFFFFF) + (a & 0xFF)])
    return bool(w >> 31), w & 0xFFFFFF


def test_statuses():
    lpm = nffacl.CreateLPM("lpm", 0, 4, 1)
    assert [lpm.Add(1, 0, 1), lpm.Add(1, 33, 1), lpm.Delete(1, 0)] == [nffacl.ERR_INVALID_ARG] * 3
    assert lpm.Add(0x0A0000FF, 8, 1) == 0 and lpm.Delete(0x0B000000, 8) == nffacl.ERR_INVALID_ARG
    assert lpm.Add(0x0A000000, 8, 0x12345678) == 0 and lpm.count() == 1   # masked ip: the same rule, hop replaced
    assert walk(lpm.compile(), 0x0A010203) == (True, 0x345678)
    assert lpm.Add(0x0A000001, 32, 2) == 0 and lpm.Add(0x0A000002, 31, 3) == 0   # one /24 block: one tbl8
    assert lpm.Add(0x0A000100, 25, 4) == nffacl.ERR_NOMEM and lpm.count() == 3    # a second block: number_tbl8
    assert lpm.Add(0x0A000004, 30, 5) == 0                                        # the first block again
    assert lpm.Add(0x0B000000, 8, 4) == nffacl.ERR_NOMEM and lpm.count() == 4     # max_rules
    assert lpm.Add(0x0A000001, 32, 9) == 0                                        # a replacement is no new rule
    assert [lpm.Delete(0x0A000001, 32), lpm.Delete(0x0A000002, 31), lpm.Delete(0x0A000004, 30)] == [0, 0, 0]
    assert lpm.Add(0x0A000100, 25, 4) == 0 and lpm.count() == 2                   # the block's budget came back
    lpm.Free()


def test_kats_through_the_compiled_table():
    play(KATS["steps"], lambda lpm, dirty, ip: walk(lpm.compile(), ip))
    rules = edge_rules()
    blob, addr = table(rules).compile(), edge_addresses(rules, 2000)
    hit, hop = reference(rules, addr)
    assert [walk(blob, int(a)) for a in addr] == [(bool(h), int(x) if h else 0) for h, x in zip(hit, hop)]


@pytest.mark.gpu
def test_kats_on_the_device(torch):
    def lookup(lpm, dirty, ip):
        if dirty:
            lpm.commit()
        out = torch.zeros(4, dtype=torch.int32, device="cuda")
        bits = torch.zeros(2, dtype=torch.int64, device="cuda")
        lpm.lookup_device(torch.tensor([ip - (1 << 32) if ip >> 31 else ip], dtype=torch.int32, device="cuda"), 1,
                          out, bits)
        return bool(bits[0].item()), out[0].item()
    play(KATS["steps"], lookup)


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [0, LPM_SWAP_BYTES])
@pytest.mark.parametrize("form", [LPM_FORCE_LDS, LPM_FORCE_GLOBAL])
@pytest.mark.parametrize("keys", [False, True])
def test_edge_table(torch, edge, keys, form, swap):
    lpm, rules, addr = edge
    cmp = check(torch, lpm, rules, addr, keys, form | swap)
    torch.cuda.synchronize()
    cmp()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [LPM_FORCE_LDS, LPM_FORCE_GLOBAL])
@pytest.mark.parametrize("keys", [False, True])
@pytest.mark.parametrize("n", [1, 3, 63, 65, 257, 4096 + 5])
def test_ragged_tails(torch, edge, n, keys, form):
    lpm, rules, addr = edge
    cmp = check(torch, lpm, rules, addr[-n:], keys, form)
    torch.cuda.synchronize()
    cmp()


@pytest.mark.gpu
@pytest.mark.parametrize("form", [LPM_FORCE_LDS, LPM_FORCE_GLOBAL])
@pytest.mark.parametrize("routes", [5000, 0])
def test_hops_past_the_codes_and_empty_table(torch, routes, form):
    """5 000 /16 routes with 5 000 distinct next hops: the leaves past the coded hops sit in level-1 groups."""
    rules = {(0x20000000 + (b << 16), 16): 100 + b for b in range(routes)}
    lpm = table(rules, max_rules=6000)
    lpm.commit()
    rng = np.random.default_rng(17)
    addr = np.concatenate([np.array([ip | 0x1234 for ip, _ in rules], np.uint32),
                           rng.integers(0, 1 << 32, 1000, dtype=np.uint32)])
    cmp = check(torch, lpm, rules, addr, flags=form)
    torch.cuda.synchronize()
    cmp()
    lpm.Free()


@pytest.mark.gpu
def test_commit_between_lookups_on_one_stream(torch, edge):
    _, rules, addr = edge
    lpm, s = table(rules), torch.cuda.Stream()
    lpm.commit()
    first = check(torch, lpm, rules, addr, stream=s)
    newer = dict(rules)
    newer[(0x0A141E00, 26)] = 77   # a prefix the first table must not know
    assert lpm.Add(0x0A141E00, 26, 77) == 0
    lpm.commit()
    second = check(torch, lpm, newer, addr, stream=s)
    s.synchronize()
    first()
    second()
    lpm.Free()


@pytest.mark.gpu
def test_invalid_arguments(torch, edge):
    lpm, _, _ = edge
    a = torch.zeros(64, dtype=torch.int32, device="cuda")
    o = torch.zeros(64, dtype=torch.int32, device="cuda")
    b = torch.zeros(4, dtype=torch.int64, device="cuda")
    fresh = nffacl.CreateLPM("lpm", 0, 4, 4)
    for who, args, kw in ((lpm, (a[1:], 8, o, b), {}), (lpm, (a, 8, o[1:], b), {}), (lpm, (a, 8, o, b[1:]), {}),
                          (lpm, (a, 8, None, None), {}), (lpm, (a, 8, o, b), {"flags": LPM_FORCE_LDS | LPM_FORCE_GLOBAL}),
                          (lpm, (a, 8, o, b), {"flags": 8}), (lpm, (a, 1 << 32, o, b), {}), (fresh, (a, 8, o, b), {})):
        for call in (who.lookup_device, who.lookup_keys_device):
            with pytest.raises(nffacl.NFError) as e:
                call(*args, **kw)
            assert e.value.status == nffacl.ERR_INVALID_ARG
    fresh.Free()
