"""hgnn_table_fingerprint (csrc/fingerprint.hip): the 64-bit checksum that HGNN_STATIC_AGG=check
keeps beside a static aggregate,

    fp(x) = sum_i bits(x[i]) * (0x9E3779B97F4A7C15 + 2 i)  (mod 2^64),

against numpy's wrapping uint64 arithmetic of the same formula.  Integer sums: the comparison is
exact.  Sizes: 1, 3 (tail only), 4 (one 16-byte lane, no tail), 64*4+1 (one wave + a tail word)
and 1,000,003 (grid-stride loop, many blocks combined by the atomic, a 3-word tail)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
K = np.uint64(0x9E3779B97F4A7C15)
SIZES = [1, 3, 4, 64 * 4 + 1, 1_000_003]


def _ref(a: np.ndarray) -> int:
    w = a.view(np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = K + np.uint64(2) * np.arange(w.size, dtype=np.uint64)
        return int((w * m).sum(dtype=np.uint64))


def _fp(t: torch.Tensor) -> int:
    from truth_recommendation_gnn_amd import ops
    return int(ops.table_fingerprint(t)) & (2**64 - 1)


def _table(n: int) -> np.ndarray:
    return np.random.default_rng(n).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_fingerprint_matches_numpy_reference(n):
    a = _table(n)
    t = torch.from_numpy(a).to(DEV)
    got = _fp(t)
    print(f"n={n}: got {got:#018x} ref {_ref(a):#018x}")
    assert got == _ref(a)
    assert _fp(t) == got                      # two runs agree (integer sums, any block order)


@pytest.mark.parametrize("n", SIZES)
def test_fingerprint_sees_one_flipped_bit_and_a_swap(n):
    a = _table(n)
    base = _fp(torch.from_numpy(a).to(DEV))
    for pos, bit in ((0, 0), (n - 1, 31), (n // 2, 13)):
        b = a.copy()
        b.view(np.uint32)[pos] ^= np.uint32(1 << bit)
        got = _fp(torch.from_numpy(b).to(DEV))
        assert got == _ref(b) and got != base, (pos, bit)
    if n >= 2:
        i, j = 0, n - 1
        b = a.copy()
        b[i], b[j] = a[j], a[i]
        assert a[i] != a[j]
        got = _fp(torch.from_numpy(b).to(DEV))
        assert got == _ref(b) and got != base


def test_fingerprint_of_a_view_off_the_16_byte_grid():
    """A table that starts 4 bytes into an allocation takes the 4-bytes-per-lane kernel: same
    formula, indices counted from the view's first word."""
    a = _table(1000)
    t = torch.from_numpy(a).to(DEV)
    for off in (1, 2, 3, 4):
        assert _fp(t[off:]) == _ref(a[off:]), off


def test_fingerprint_rejects_what_it_cannot_read():
    from truth_recommendation_gnn_amd import ops
    with pytest.raises(TypeError):
        ops.table_fingerprint(torch.zeros(4, dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError):
        ops.table_fingerprint(torch.zeros(4, 4, device=DEV).t())
    assert _fp(torch.zeros(0, device=DEV)) == 0
