"""Packed-frame gather (csrc/route_frames.hip), exact against a numpy packing of the same frames."""
import numpy as np
import pytest

import nffacl
from nffacl import synth
from oracle import oracle, rules_oracle as ro

T = (1 << 20) // nffacl.route_frames_plan(1 << 20)[0]  # frames per tile
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 37]
SHAPES = [(m, lens, False) for m in SIZES for lens in ("imix", "ragged", "max") if lens != "max" or m <= 65]
SHAPES += [(3 * T + 37, "imix", True), (3 * T + 37, "ragged", True), (65, "max", True)]  # out_cap = half the bytes


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no HIP device")
    return t


def batch(lens, n, seed):  # n random frames in 64-byte rooms, every room 0xA5 past its frame's length
    rng = np.random.default_rng(seed)
    ln = {"imix": rng.choice([64, 570, 1518], n, p=[7 / 12, 4 / 12, 1 / 12]), "ragged": rng.integers(0, 1519, n),
          "max": np.full(n, 65535)}[lens].astype(np.int64)
    room = (ln + 63) // 64 * 64
    off = np.cumsum(room) - room
    frames = rng.integers(0, 256, int(room.sum()), dtype=np.uint8)
    frames[np.arange(len(frames)) - np.repeat(off, room) >= np.repeat(ln, room)] = 0xA5
    return frames, off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64)


def indices(pattern, n, m, seed):
    if pattern == "random":  # repeats, about 1 % past the batch
        rng = np.random.default_rng(seed)
        idx = rng.integers(0, n, m)
        bad = rng.random(m) < 0.01
        idx[bad] = rng.choice([n, n + 1, 0xFFFFFFFF], int(bad.sum()))
        return idx.astype(np.uint32)
    return np.arange(m, dtype=np.uint32)[::-1 if pattern == "reversed" else 1].copy()


def pack(frames, desc, index, align):  # (bytes, descriptors, total) of the packed batch, as nffacl.h defines it
    d = np.where(index < len(desc), desc[np.minimum(index, len(desc) - 1)], 0).astype(np.int64)
    ln, src = d & 0xFFFF, d >> 16
    room = (ln + align - 1) // align * align
    off = np.cumsum(room) - room
    out = np.zeros(int(room.sum()), np.uint8)
    within = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    out[np.repeat(off, ln) + within] = frames[np.repeat(src, ln) + within]
    return out, off.astype(np.uint64) << np.uint64(16) | ln.astype(np.uint64), len(out)


def launch(torch, router, frames, desc, index, align, short=False):  # launch only; guards behind d_out, out_desc
    want = pack(frames, desc, index, align)
    cap = want[2] // 2 // 16 * 16 if short else want[2]
    assert not short or 0 < cap < want[2]
    dev = [torch.from_numpy(a.view(t)).to("cuda") for a, t in ((frames, np.uint8), (desc, np.int64), (index, np.int32))]
    out = torch.full((want[2] + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out_desc = torch.full((len(index) + 1,), -1, dtype=torch.int64, device="cuda")
    out_bytes = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    router.gather_frames(dev[0], dev[1], len(desc), dev[2], len(index), out, cap, out_desc, out_bytes, align)
    return want, cap, out, out_desc, out_bytes, dev


def check(want, cap, out, out_desc, out_bytes, _):
    got, gd = out.cpu().numpy(), out_desc.cpu().numpy().view(np.uint64)
    assert int(out_bytes.cpu()[0]) == want[2] and gd[-1] == 0xFFFFFFFFFFFFFFFF
    np.testing.assert_array_equal(gd[:-1], want[1])
    np.testing.assert_array_equal(got[:cap], want[0][:cap])  # data, clipped tails, zero pads
    assert (got[cap:] == 0xEE).all()  # nothing at or past out_cap, nor in the guard


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["identity", "reversed", "random"])
@pytest.mark.parametrize("align", [16, 64])
@pytest.mark.parametrize("m,lens,short", SHAPES)
def test_gather_frames_matches_packing(torch, m, lens, short, align, pattern):
    frames, desc = batch(lens, max(m, 1), m)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, max(m, 1)) as r:
        res = launch(torch, r, frames, desc, indices(pattern, len(desc), m, m + 1), align, short)
        torch.cuda.synchronize()
    check(*res)


@pytest.mark.gpu
def test_gather_frames_reuses_scratch(torch):  # large, small, large through one router, in stream order
    big, small = batch("imix", 3 * T + 37, 7), batch("ragged", 65, 8)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, 3 * T + 37) as r:
        runs = [launch(torch, r, *b, indices("random", len(b[1]), len(b[1]), 9), 64) for b in (big, small, big)]
        torch.cuda.synchronize()
    for res in runs:
        check(*res)


@pytest.mark.gpu
def test_classify_route_gather_frames(torch, golden):
    """The per-output packed frames classify to the verdicts that routed them."""
    text, n = (golden / "rules" / "forwarding.conf").read_text(), 3 * T + 37
    frames, desc = synth.gen_imix(synth.firewall_rules(text), n, 11)
    a4, a6 = ro.parse_text_table(text.encode()).arrays()
    want = oracle.classify_frames(frames, desc, a4, a6, threads=8)
    n_out = int(want.max()) + 1
    assert len(set(want.tolist())) >= 4
    d_frames, d_desc = torch.from_numpy(frames).to("cuda"), torch.from_numpy(desc.view(np.int64)).to("cuda")
    port, port2, index = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    offsets = torch.zeros(n_out + 2, dtype=torch.int32, device="cuda")
    out = torch.zeros(len(frames), dtype=torch.uint8, device="cuda")
    out_desc, out_bytes = (torch.zeros(k, dtype=torch.int64, device="cuda") for k in (n, 1))
    with nffacl.Engine(nffacl.L3Rules.parse_text(text)) as eng, nffacl.Router(nffacl.ROUTE_SPLIT, n_out, n) as r:
        eng.classify_frames_device(d_frames, d_desc, n, port)
        r.route(port, n, index, offsets)
        r.gather_frames(d_frames, d_desc, n, index, n, out, len(frames) // 16 * 16, out_desc, out_bytes)
        eng.classify_frames_device(out, out_desc, n, port2)
        torch.cuda.synchronize()
    got, got2, off = port.cpu().numpy().view(np.uint32), port2.cpu().numpy().view(np.uint32), offsets.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got2, want[index.cpu().numpy()])
    assert int(out_bytes.cpu()[0]) <= len(frames) and off[n_out] == n  # it fitted; no out-of-range answers
    assert all((got2[off[o]:off[o + 1]] == o).all() for o in range(n_out))  # one output per segment


@pytest.mark.gpu
def test_gather_frames_rejects_bad_arguments(torch):
    frames, desc = batch("imix", 64, 3)
    out = torch.full((1 << 17,), 0xEE, dtype=torch.uint8, device="cuda")
    od, ob = (torch.full((k,), -1, dtype=torch.int64, device="cuda") for k in (65, 1))
    good = [torch.from_numpy(frames).to("cuda"), torch.from_numpy(desc.view(np.int64)).to("cuda"), 64,
            torch.arange(64, dtype=torch.int32, device="cuda"), 64, out, 1 << 17, od, ob, 64]
    # (argument, value): align; out_cap % 16; m > max_n; NULL frames, desc, index, out, out_desc, out_bytes
    bad = [(9, 0), (9, 8), (9, 24), (9, 8192), (6, (1 << 17) - 8), (4, 65)] + [(k, None) for k in (0, 1, 3, 5, 7, 8)]
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, 64) as r:
        for k, v in bad:
            with pytest.raises(nffacl.NFError) as e:
                r.gather_frames(*good[:k], v, *good[k + 1:])
            assert e.value.status == nffacl.ERR_INVALID_ARG
        torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xEE).all() and (od.cpu().numpy() == -1).all() and int(ob.cpu()[0]) == -1  # no launch
