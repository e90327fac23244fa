"""Guard bands, bit-exact snapshots and workspace poison for the C-ABI buffer-contract tests (device-agnostic: the
checker itself is tested on CPU tensors in tests/test_abi_contract_util_cpu.py).

Poison is the FINITE float 1e30 everywhere (float32 0x7149F2CA; as a double for float64 buffers), never NaN and never an
all-ones pattern: a poisoned value that a kernel multiplies by an exact zero (masked tail lanes) stays harmless, and read
as an integer it is a large positive number, not -1.  Integer buffers are filled with 0x7149F2CA7149F2CA (the float
pattern twice); uint8 buffers with the four bytes of the float, so that a workspace viewed as float32 holds 1e30."""
import torch

POISON = 1e30
INT64_POISON = 0x7149F2CA7149F2CA
BAND = 64          # elements in front of and behind the payload; at least 256 bytes, so the payload keeps torch's alignment

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    """The tensor's elements as integers of the same size (flat): what 'bit for bit' compares."""
    t = t.detach().contiguous().reshape(-1)
    return t if t.dtype in (torch.uint8, torch.int16, torch.int32, torch.int64) else t.view(_BITS[t.element_size()])


def band_elements(dtype):
    """64 elements, or as many as make 256 bytes for the one-byte type (the workspace)."""
    return max(BAND, 256 // torch.empty(0, dtype=dtype).element_size())


def _poison_fill(flat):
    """Fill a flat buffer (length a multiple of 4 bytes) with the poison of its dtype."""
    if flat.dtype == torch.uint8:
        flat.view(torch.float32).fill_(POISON)
    elif flat.dtype == torch.int64:
        flat.fill_(INT64_POISON)
    elif flat.dtype == torch.int32:
        flat.fill_(0x7149F2CA)
    elif flat.dtype.is_floating_point:
        flat.fill_(POISON)
    else:
        raise TypeError(f"no poison for {flat.dtype}")


class GuardChecker:
    """Remembers the poison of both bands of one guarded buffer; offsets are reported in elements relative to the
    payload's first element (-1 = the element just in front, numel = the element just behind)."""

    def __init__(self, flat, front, numel, name=""):
        self.flat, self.front, self.numel, self.name = flat, front, numel, name
        self._want_front = _bits(flat[:front]).clone()
        self._want_back = _bits(flat[front + numel:]).clone()

    def first_touched(self):
        """Offset of the first band element that no longer holds the poison, or None."""
        bad = (_bits(self.flat[:self.front]) != self._want_front).nonzero()
        if bad.numel():
            return int(bad[0]) - self.front
        bad = (_bits(self.flat[self.front + self.numel:]) != self._want_back).nonzero()
        if bad.numel():
            return self.numel + int(bad[0])
        return None

    def assert_bands_intact(self):
        off = self.first_touched()
        assert off is None, (f"guard band of {self.name or 'buffer'} touched at offset {off} "
                             f"(payload is [0, {self.numel}); value there now {self.flat[self.front + off].item()!r})")


def guarded(shape, dtype=torch.float32, device="cpu", fill=None, name=""):
    """One flat allocation [front band | payload | back band], everything poisoned; returns (payload view of `shape`,
    GuardChecker).  fill: value the payload is set to instead of the poison."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    numel = 1
    for s in shape:
        numel *= int(s)
    band = band_elements(dtype)
    pad = (-numel) % 4 if dtype == torch.uint8 else 0          # (the byte buffer is poisoned through a float32 view)
    flat = torch.empty(band + numel + band + pad, dtype=dtype, device=device)
    _poison_fill(flat)
    payload = flat[band:band + numel].view(shape)
    if fill is not None:
        payload.fill_(fill)
    return payload, GuardChecker(flat, band, numel, name)


def snapshot(t):
    """Bit-exact copy of a read-only argument, taken before the call."""
    return _bits(t).clone()


def assert_unchanged(t, snap, name=""):
    now = _bits(t)
    assert now.shape == snap.shape, f"{name or 'argument'} changed size"
    bad = (now != snap).nonzero()
    assert bad.numel() == 0, f"read-only {name or 'argument'} was written: first changed element {int(bad[0])} of {now.numel()}"


def poison_workspace(ws):
    """Fill a uint8 workspace tensor, viewed as float32, with 1e30 (a tail of fewer than four bytes gets the float's
    first bytes)."""
    assert ws.dtype == torch.uint8 and ws.is_contiguous()
    n4 = ws.numel() // 4 * 4
    if n4:
        ws[:n4].view(torch.float32).fill_(POISON)
    if ws.numel() > n4:
        pat = torch.tensor([POISON], dtype=torch.float32).view(torch.uint8)
        ws[n4:] = pat[:ws.numel() - n4].to(ws.device)
    return ws
