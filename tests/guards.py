"""Guard bands for the memory-discipline tests (tests/test_gpu_guards*.py): every tensor a kernel is given lives in one flat buffer of its own,

    [ front band | rows x ld payload (logical columns col_off .. col_off + cols, the rest is row padding) | back band ]

whose bands and padding hold a chosen byte pattern.  After the call an INPUT buffer must be bit-identical to before (payload, padding and bands);
of an OUTPUT buffer only the logical elements may have changed, and (results that are finite) every one of them must have been written: they start
as NaN.  Two fills exist so that one call can be run twice and its logical outputs compared bit for bit: 0xFF bytes (NaN in f32, bf16 and fp16, -1 in
the integer types) and 0x47 bytes (f32 51015.28, bf16 50944, fp16 7.277, a large non-zero integer).  A result that differs between the two depends
on bytes the kernel was never given.

A band is at least 256 rows of the tensor's leading dimension and never less than 64 KiB: an edge tile, a vector access at a ragged edge or a scratch
row too many of a kernel that is wrong lands in memory the test owns, so these tests cannot fault the device.  Works on CPU tensors too (the helper's
own tests run without a GPU).  A plain module: no fixtures, no pytest settings."""
import torch

FILLS = {"nan": 0xFF, "finite": 0x47}
NAN_BYTE = 0xFF
BAND_ROWS = 256
BAND_MIN_BYTES = 64 * 1024
_FLOAT = (torch.float32, torch.bfloat16, torch.float16, torch.float64)


class GuardViolation(AssertionError):
    pass


def _round_up(v, m):
    return (v + m - 1) // m * m


def band_bytes(ld, elt):
    return _round_up(max(BAND_ROWS * ld * elt, BAND_MIN_BYTES), 256)


class Guarded:
    """One guarded tensor.  `view`: the logical [rows, cols] tensor (row stride ld); `ptr` / `ld`: what the C call takes."""

    def __init__(self, name, role, rows, cols, dtype, ld, col_off, misalign, fill, device, data=None, init=None, written=True, band=None):
        assert role in ("in", "out", "scratch")
        ld = cols + col_off if ld is None else ld
        assert rows >= 1 and cols >= 1 and ld >= col_off + cols and misalign >= 0
        self.name, self.role, self.rows, self.cols, self.dtype, self.ld, self.col_off = name, role, rows, cols, dtype, ld, col_off
        self.elt = torch.empty((), dtype=dtype).element_size()
        assert misalign % self.elt == 0
        self.fill, self.written = fill, written and role == "out" and dtype in _FLOAT
        band = band_bytes(ld, self.elt) if band is None else _round_up(max(band, BAND_MIN_BYTES), 256)
        self.front = band + misalign                      # the allocation is 256-byte aligned, so is the band: payload alignment = misalign
        self.payload_bytes = rows * ld * self.elt
        self.back = band
        self.buf = torch.full((self.front + self.payload_bytes + self.back,), fill, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % 256 == 0 or torch.device(device).type == "cpu"
        self.view = self.buf[self.front:self.front + self.payload_bytes].view(dtype).view(rows, ld)[:, col_off:col_off + cols]
        if role == "in":
            assert data is not None and tuple(data.shape) == (rows, cols), (name, tuple(data.shape), rows, cols)
            self.view.copy_(data.to(dtype))
        elif init is not None:                            # an output the header documents as ACCUMULATED starts from known values
            self.view.copy_(init.to(dtype).reshape(rows, cols))
        elif role == "out":                               # every logical element must be written: start from NaN (-1 for integers) under either fill
            self._logical_bytes().fill_(NAN_BYTE)
        self.ptr = self.view.data_ptr()
        self.before = self.buf.clone()

    def _logical_bytes(self, buf=None):
        buf = self.buf if buf is None else buf
        e = self.elt
        return buf[self.front:self.front + self.payload_bytes].view(self.rows, self.ld * e)[:, self.col_off * e:(self.col_off + self.cols) * e]

    def regions(self):
        """Byte counts that differ from the state before the call, per region."""
        diff = self.buf != self.before
        mid = diff[self.front:self.front + self.payload_bytes].view(self.rows, self.ld * self.elt)
        logical = int(self._logical_bytes(diff).sum())
        return {"front band": int(diff[:self.front].sum()), "back band": int(diff[self.front + self.payload_bytes:].sum()),
                "row padding": int(mid.sum()) - logical, "payload": logical}

    def first_diff(self, region):
        diff = self.buf != self.before
        if region == "payload":
            d = torch.zeros_like(diff); self._logical_bytes(d).copy_(self._logical_bytes(diff)); diff = d
        elif region == "row padding":
            diff = diff.clone(); self._logical_bytes(diff).fill_(False); diff[:self.front] = False; diff[self.front + self.payload_bytes:] = False
        elif region == "front band":
            diff = diff.clone(); diff[self.front:] = False
        else:
            diff = diff.clone(); diff[:self.front + self.payload_bytes] = False
        idx = int(torch.nonzero(diff)[0])
        return idx - self.front                           # byte offset relative to the payload start (negative: in the front band)

    def violations(self):
        out = []
        r = self.regions()
        checked = ("front band", "back band", "row padding") + (("payload",) if self.role == "in" else ())
        for region in checked:
            if r[region]:
                what = "input" if self.role == "in" else ("scratch" if self.role == "scratch" else "output")
                out.append(f"{self.name}: {what} {region} changed ({r[region]} bytes, first at byte {self.first_diff(region):+d} of the payload; "
                           f"rows {self.rows}, cols {self.cols}, ld {self.ld}, col_off {self.col_off}, {self.dtype})")
        if self.written:
            bad = torch.isnan(self.view.float())
            if bool(bad.any()):
                i = torch.nonzero(bad)[0].tolist()
                out.append(f"{self.name}: output payload has {int(bad.sum())} NaN logical elements (never written, or computed from bytes outside "
                           f"the inputs), first at {i}; rows {self.rows}, cols {self.cols}, ld {self.ld}")
        return out


class GuardSet:
    """All the guarded tensors of one call under one fill."""

    def __init__(self, fill, device="cuda"):
        self.fill_name, self.fill, self.device = fill, FILLS[fill], device
        self.tensors = []

    def _add(self, g):
        self.tensors.append(g)
        return g

    def inp(self, name, data, ld=None, col_off=0, misalign=0):
        """Input [rows, cols] (a 1-D tensor is one row).  ld > cols: padded rows; col_off > 0: a column slice of a wider buffer."""
        data = data.reshape(1, -1) if data.dim() == 1 else data.reshape(-1, data.shape[-1])
        return self._add(Guarded(name, "in", data.shape[0], data.shape[1], data.dtype, ld, col_off, misalign, self.fill, self.device, data=data))

    def out(self, name, rows, cols, dtype, ld=None, col_off=0, misalign=0, init=None, written=True):
        return self._add(Guarded(name, "out", rows, cols, dtype, ld, col_off, misalign, self.fill, self.device, init=init, written=written))

    def scratch(self, name, nbytes, row_bytes=0, zero=False):
        """Scratch of EXACTLY nbytes (the library's capacity function's answer); contents free, bands checked.  A flat byte region has no leading
        dimension of its own: `row_bytes` is the longest row of what is laid out inside it (bands: 256 of those, at least 64 KiB).  Starts as the
        fill; zero: as zeros (bands keep the fill)."""
        g = Guarded(name, "scratch", 1, max(int(nbytes), 1), torch.uint8, None, 0, 0, self.fill, self.device, band=BAND_ROWS * row_bytes)
        if zero:
            g.view.zero_(); g.before = g.buf.clone()
        return self._add(g)

    def violations(self):
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        return [f"[{self.fill_name} fill] {v}" for g in self.tensors for v in g.violations()]

    def check(self):
        v = self.violations()
        if v:
            raise GuardViolation("\n".join(v))


def assert_bit_identical(a, b, what=""):
    """Logical outputs of the same call under the two fills."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ia, ib = a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)
    if not torch.equal(ia, ib):
        n = int((a != b).sum()) if a.dtype in _FLOAT else int((ia != ib).sum())
        d = float((a.double() - b.double()).abs().max()) if a.dtype in _FLOAT else -1.0
        raise GuardViolation(f"{what}: logical output differs between the NaN fill and the finite fill ({n} elements, max |diff| {d:.3e}): "
                             f"the result depends on bytes outside the logical inputs")
