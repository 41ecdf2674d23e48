"""bench.py --dump-outputs on host tensors (no GPU): whole batch below the
packet limit, the fixed seeded sample above it."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def _buffers(n):
    rng = np.random.default_rng(5)
    port = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    words = rng.integers(0, 1 << 63, (n + 63) // 64, dtype=np.uint64) << np.uint64(1) | np.uint64(1)
    return port, words, torch.from_numpy(port.view(np.int32)), torch.from_numpy(words.view(np.int64))


def _check_words(path, words):
    got = np.load(path / "permit_bits.npy")
    assert got.dtype == np.float64 and got.shape == (len(words), 2)
    assert (got[:, 0].astype(np.uint64) | got[:, 1].astype(np.uint64) << np.uint64(32) == words).all()


def test_dump_small_batch_is_whole_and_exact(tmp_path):
    n = 1000
    port, words, t_port, t_words = _buffers(n)
    bench.dump_outputs(str(tmp_path / "a" / "b"), t_port, t_words, n)
    got = np.load(tmp_path / "a" / "b" / "port.npy")
    assert got.dtype == np.float64 and (got == port).all() and got.shape == (n,)
    _check_words(tmp_path / "a" / "b", words)


def test_dump_large_batch_is_a_fixed_sample(tmp_path):
    n = bench.DUMP_MAX_PACKETS + 4097
    port, words, t_port, t_words = _buffers(n)
    bench.dump_outputs(str(tmp_path / "x"), t_port, t_words, n)
    bench.dump_outputs(str(tmp_path / "y"), t_port, t_words, n)
    x, y = np.load(tmp_path / "x" / "port.npy"), np.load(tmp_path / "y" / "port.npy")
    assert x.shape == (bench.DUMP_MAX_PACKETS,) and (x == y).all()
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, bench.DUMP_MAX_PACKETS, replace=False))
    assert (x == port[idx]).all()
    _check_words(tmp_path / "x", words)
    total = sum(f.stat().st_size for f in (tmp_path / "x").iterdir())
    assert total <= 64 * 1000 * 1000
