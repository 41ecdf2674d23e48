"""Keys from packed frames (csrc/keys.hip) against extract_keys_host, their verdicts against the oracle."""
import numpy as np
import pytest

import nffacl
from oracle import oracle, rules_oracle as ro

N = 4099
TEXT = "\n".join(f"ANY ANY {p} {a}:{b} {c}:{d} {o}" for p, a, b, c, d, o in [
    ("TCP", 0, 30000, 0, 65535, 2), ("UDP", 20000, 65535, 100, 40000, 3), ("ANY", 0, 0, 0, 65535, 4),
    ("ANY", 0, 65535, 0, 0, 5), ("ANY", 1000, 50000, 1000, 50000, 6)]) + "\n"


@pytest.fixture(scope="module")
def frames_batch():
    # IHL 0..15, every other 16 frames 802.1Q-tagged, lengths 128 / 80 / 64 / 61 / 40, one frame in eight IPv6
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    rng = np.random.default_rng(13)
    buf, desc, off = [], [], 0
    for i in range(N):
        f = bytearray(rng.integers(0, 256, 132, dtype=np.uint8).tobytes())
        f[12:14] = b"\x86\xdd" if i % 8 == 5 else b"\x08\x00"
        f[14] = 0x40 | (i % 16)
        f[20 if i % 8 == 5 else 23] = [6, 17, 1][i % 3]
        if (i // 16) % 2:
            f = f[:12] + bytearray(b"\x81\x00\x00\x05") + f[12:128]
        ln = [128, 80, 64, 61, 40][(i // 32) % 5]
        buf.append(bytes(f[:ln]) + bytes(-ln % 64))  # 64-byte rooms
        desc.append(off << 16 | ln)
        off += len(buf[-1])
    return torch, np.frombuffer(b"".join(buf), np.uint8).copy(), np.array(desc, np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, nffacl.PARSE_VLAN])
@pytest.mark.parametrize("n", [1, 63, 64, 65, N])
def test_keys_from_frames(frames_batch, n, flags):
    torch, frames, desc = frames_batch[0], frames_batch[1], frames_batch[2][:n]
    keys = torch.full((n, 4), -1, dtype=torch.int32, device="cuda")
    key6 = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    port = torch.zeros(n, dtype=torch.int32, device="cuda")
    a4, a6 = ro.parse_text_table(TEXT.encode()).arrays()
    with nffacl.Engine(nffacl.L3Rules.parse_text(TEXT)) as eng:
        nffacl.extract_keys_frames_device(torch.from_numpy(frames).to("cuda"),
                                          torch.from_numpy(desc.view(np.int64)).to("cuda"), n, keys, key6, flags)
        eng.classify_keys_device(keys, key6, n, n, port)
        torch.cuda.synchronize()
    got, got6 = (t.cpu().numpy().view(d).reshape(-1) for t, d in ((keys, nffacl.KEY_DTYPE), (key6, nffacl.KEY6_DTYPE)))
    want, want6 = nffacl.extract_keys_host(np.uint64(frames.ctypes.data) + (desc >> np.uint64(16)),
                                           (desc & np.uint64(0xFFFF)).astype(np.uint32), flags)
    six = (want["meta"] >> 8) == 6
    for field in ("b", "ports", "meta"):
        np.testing.assert_array_equal(got[field], want[field])
    np.testing.assert_array_equal(got["a"][~six], want["a"][~six])
    np.testing.assert_array_equal(got["a"][six], np.nonzero(six)[0])  # an IPv6 record lies at its frame's index
    np.testing.assert_array_equal(got6[got["a"][six]], want6[want["a"][six]])
    verdicts = oracle.classify_frames(frames, desc, a4, a6, flags=flags)
    assert n < N or len(set(verdicts.tolist())) > 3
    np.testing.assert_array_equal(port.cpu().numpy().view(np.uint32), verdicts)
