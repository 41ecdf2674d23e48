"""Routing stage (nffacl_router_*, csrc/route.hip): the per-output index lists
segmentProcess builds per burst (flow/flow.go:1462-1486), checked for exact
integer equality against numpy's stable partition of the same keys."""
import numpy as np
import pytest

import nffacl
from nffacl import synth
from oracle import oracle, rules_oracle as ro

T = (1 << 24) // nffacl.route_plan(1 << 24, 2)[0]  # keys per tile
MODES = [(nffacl.ROUTE_SEPARATE, 2), (nffacl.ROUTE_SPLIT, 1), (nffacl.ROUTE_SPLIT, 3), (nffacl.ROUTE_SPLIT, 5),
         (nffacl.ROUTE_SPLIT, 255)]
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 37]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def ports(pattern, n, n_out):
    i = np.arange(n, dtype=np.int64)
    if pattern == "same":
        p = np.full(n, n_out - 1)
    elif pattern == "cycle":
        p = i % n_out
    elif pattern == "runs":  # runs straddle tiles; some outputs are empty inside a tile
        p = (i // (T + 1)) % n_out
    else:  # uniform, about 1 % out of range
        rng = np.random.default_rng(n * 256 + n_out)
        p = rng.integers(0, n_out, n)
        bad = rng.random(n) < 0.01
        p[bad] = rng.choice([n_out, n_out + 1, 0xFFFFFFFF], int(bad.sum()))
        p[n // 2:n // 2 + (n >= 64)] = 0xFFFFFFFF
    return p.astype(np.uint32)


def partition(mode, port, n_out):
    """(index, offsets) of the reference: OutputMbufs[0], [1], ... laid end to end."""
    key = (port != 0) if mode == nffacl.ROUTE_SEPARATE else port
    k = np.minimum(key, n_out).astype(np.int64)
    offsets = np.concatenate(([0], np.cumsum(np.bincount(k, minlength=n_out + 1))))
    return np.argsort(k, kind="stable").astype(np.uint32), offsets.astype(np.uint32)


def route(torch, router, port, n_out):
    """Launch only; index has one guard word past n."""
    n = len(port)
    d_port = torch.from_numpy(port.view(np.int32)).to("cuda")
    index = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    offsets = torch.full((n_out + 2,), -1, dtype=torch.int32, device="cuda")
    router.route(d_port, n, index, offsets)
    return d_port, index, offsets


def check(mode, port, n_out, index, offsets):
    want_index, want_offsets = partition(mode, port, n_out)
    got = index.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(offsets.cpu().numpy().view(np.uint32), want_offsets)
    np.testing.assert_array_equal(got[:-1], want_index)
    assert got[-1] == 0xFFFFFFFF  # nothing written past n


@pytest.mark.parametrize("n_out", [2, 5])
def test_route_plan(n_out):
    for n in (0, 1, T, T + 1, 1 << 24):
        tiles, scratch = nffacl.route_plan(n, n_out)
        assert tiles == -(-n // T) and scratch == tiles * (n_out + 1) * 4
    for bad in ((1 << 31) + 1, n_out), (10, 0), (10, 256):
        with pytest.raises(nffacl.NFError) as e:
            nffacl.route_plan(*bad)
        assert e.value.status == nffacl.ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["same", "cycle", "runs", "random"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mode,n_out", MODES)
def test_route_matches_stable_partition(torch_cuda, mode, n_out, n, pattern):
    port = ports(pattern, n, n_out)
    with nffacl.Router(mode, n_out, max(n, 1)) as r:
        _, index, offsets = route(torch_cuda, r, port, n_out)
        torch_cuda.cuda.synchronize()
    check(mode, port, n_out, index, offsets)


@pytest.mark.gpu
def test_route_reuses_scratch(torch_cuda):
    """Two batches of different tile counts through one router's scratch, in
    stream order with no synchronise between them."""
    big, small = ports("random", 3 * T + 37, 5), ports("cycle", 65, 5)
    with nffacl.Router(nffacl.ROUTE_SPLIT, 5, len(big)) as r:
        a = route(torch_cuda, r, big, 5)
        b = route(torch_cuda, r, small, 5)
        torch_cuda.cuda.synchronize()
    check(nffacl.ROUTE_SPLIT, big, 5, *a[1:])
    check(nffacl.ROUTE_SPLIT, small, 5, *b[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["test-split.conf", "forwarding.conf"])
def test_classify_route_gather(torch_cuda, golden, name):
    torch = torch_cuda
    text = (golden / "rules" / name).read_text()
    n = (1 << 14) + 5
    slots = synth.gen_slots(synth.firewall_rules(text), n, 11)
    a4, a6 = ro.parse_text_table(text.encode()).arrays()
    want = oracle.classify_slots(slots, 64, n, a4, a6, threads=8)
    n_split = int(max(a4["output_number"].max(), a6["output_number"].max())) + 1
    d_slots = torch.from_numpy(slots).to("cuda")
    port = torch.zeros(n, dtype=torch.int32, device="cuda")
    with nffacl.Engine(nffacl.L3Rules.parse_text(text)) as eng:
        eng.classify_device(d_slots, 64, n, port)
        for mode, n_out in ((nffacl.ROUTE_SPLIT, n_split), (nffacl.ROUTE_SEPARATE, 2)):
            index = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
            offsets = torch.zeros(n_out + 2, dtype=torch.int32, device="cuda")
            out = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            with nffacl.Router(mode, n_out, n) as r:
                r.route(port, n, index, offsets)
                r.gather(d_slots, 64, index, n, out)
                torch.cuda.synchronize()
            check(mode, want, n_out, index, offsets)
            want_index = partition(mode, want, n_out)[0]
            np.testing.assert_array_equal(out.cpu().numpy().reshape(n, 64), slots.reshape(n, 64)[want_index])


@pytest.mark.gpu
def test_route_rejects_bad_arguments(torch_cuda):
    torch = torch_cuda
    for n_out in (0, 256):
        with pytest.raises(nffacl.NFError) as e:
            nffacl.Router(nffacl.ROUTE_SPLIT, n_out, 64)
        assert e.value.status == nffacl.ERR_INVALID_ARG
    buf = torch.full((256,), 7, dtype=torch.int32, device="cuda")
    index, offsets = buf[:128], buf[128:]
    port = torch.zeros(128, dtype=torch.int32, device="cuda")
    out = torch.zeros(128 * 80, dtype=torch.uint8, device="cuda")
    with nffacl.Router(nffacl.ROUTE_SPLIT, 3, 64) as r:
        calls = [lambda: r.route(port, 65, index, offsets),                 # n > max_n
                 lambda: r.route(port, 64, None, offsets),                  # NULL d_index
                 lambda: r.gather(out, 72, index, 8, out.clone())]          # stride % 16 != 0
        for call in calls:
            with pytest.raises(nffacl.NFError) as e:
                call()
            assert e.value.status == nffacl.ERR_INVALID_ARG
        torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 7).all()  # nothing launched
