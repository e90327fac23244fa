"""tests/abi_contract_util.py can fail: a guard-band checker that never fires proves nothing on the GPU."""
import struct

import pytest
import torch

from tests.abi_contract_util import (BAND, INT64_POISON, POISON, assert_unchanged, band_elements, guarded, poison_workspace,
                                     snapshot)

DTYPES = [torch.float32, torch.float64, torch.int64, torch.uint8]


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_layout_and_poison(dtype):
    t, chk = guarded((3, 5), dtype)
    band = band_elements(dtype)
    assert t.shape == (3, 5) and t.dtype == dtype and t.is_contiguous()
    assert band >= BAND and band * t.element_size() % 256 == 0
    assert t.data_ptr() - chk.flat.data_ptr() == band * t.element_size()
    assert chk.flat.numel() >= 15 + 2 * band
    if dtype == torch.int64:
        assert bool((chk.flat == INT64_POISON).all())
    elif dtype == torch.uint8:
        assert bool((chk.flat.view(torch.float32) == POISON).all())
    else:
        assert bool((chk.flat == POISON).all()) and bool(torch.isfinite(chk.flat).all())
    chk.assert_bands_intact()
    z, chk0 = guarded(7, dtype, fill=0)
    assert bool((z == 0).all())
    chk0.assert_bands_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_a_write_one_element_before_the_payload_is_reported(dtype):
    t, chk = guarded(10, dtype, name="Y")
    chk.flat[chk.front - 1] = 0
    assert chk.first_touched() == -1
    with pytest.raises(AssertionError, match=r"guard band of Y touched at offset -1 "):
        chk.assert_bands_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_a_write_one_element_after_the_payload_is_reported(dtype):
    t, chk = guarded((2, 5), dtype, name="dY")
    chk.flat[chk.front + 10] = 1
    assert chk.first_touched() == 10
    with pytest.raises(AssertionError, match=r"guard band of dY touched at offset 10 "):
        chk.assert_bands_intact()


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_a_write_at_the_last_band_element_is_reported(dtype):
    t, chk = guarded(10, dtype)
    last = chk.flat.numel() - 1
    chk.flat[last] = 3
    assert chk.first_touched() == last - chk.front
    with pytest.raises(AssertionError, match=rf"touched at offset {last - chk.front} "):
        chk.assert_bands_intact()
    t2, chk2 = guarded(10, dtype)
    chk2.flat[0] = 3                                   # ... and the first one
    assert chk2.first_touched() == -chk2.front


def test_the_first_of_several_touched_offsets_is_named():
    t, chk = guarded(10)
    chk.flat[chk.front + 12] = 0
    chk.flat[chk.front + 11] = 0
    assert chk.first_touched() == 11
    chk.flat[5] = 0
    assert chk.first_touched() == 5 - chk.front


def test_rewriting_the_poison_value_itself_is_not_a_touch_but_its_neighbour_in_bits_is():
    t, chk = guarded(4)
    chk.flat[chk.front + 4] = POISON                   # same bits: indistinguishable from no write (a limit of the method)
    chk.assert_bands_intact()
    nxt = struct.unpack("f", struct.pack("I", 0x7149F2CB))[0]
    chk.flat[chk.front + 4] = nxt                      # one ulp away
    assert chk.first_touched() == 4


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_payload_only_writes_pass(dtype):
    t, chk = guarded((4, 6), dtype)
    t.fill_(7)
    t[0, 0] = 1
    t[3, 5] = 2
    chk.assert_bands_intact()
    assert chk.first_touched() is None
    e, chk_e = guarded((0, 3), dtype)                  # an empty payload: the two bands touch
    assert e.numel() == 0
    chk_e.assert_bands_intact()


def test_assert_unchanged_catches_a_one_ulp_change():
    x = torch.linspace(-1, 1, 33)
    snap = snapshot(x)
    assert_unchanged(x, snap, "X")
    x[17] = torch.nextafter(x[17], torch.tensor(2.0))
    with pytest.raises(AssertionError, match=r"read-only X was written: first changed element 17 of 33"):
        assert_unchanged(x, snap, "X")
    d = torch.linspace(-1, 1, 9, dtype=torch.float64)
    snap = snapshot(d)
    d[8] = torch.nextafter(d[8], torch.tensor(2.0, dtype=torch.float64))
    with pytest.raises(AssertionError, match=r"first changed element 8"):
        assert_unchanged(d, snap)
    z = torch.zeros(3)
    snap = snapshot(z)
    z[1] = -0.0                                        # equal as a float, another bit pattern
    with pytest.raises(AssertionError, match=r"first changed element 1"):
        assert_unchanged(z, snap)


def test_snapshot_is_a_copy():
    x = torch.ones(5)
    snap = snapshot(x)
    x[0] = 2
    assert int(snap[0]) == 0x3F800000


def test_poison_workspace():
    for n in (0, 3, 256, 1030):
        ws, chk = guarded(n, torch.uint8, fill=0)
        poison_workspace(ws)
        chk.assert_bands_intact()
        assert bool((ws[:n // 4 * 4].view(torch.float32) == POISON).all())
        if n % 4:
            assert ws[n // 4 * 4:].tolist() == list(struct.pack("f", POISON))[:n % 4]
    assert struct.unpack("i", struct.pack("f", POISON))[0] == 0x7149F2CA > 0
