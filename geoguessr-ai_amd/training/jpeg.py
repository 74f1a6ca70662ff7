"""Baseline JPEG decoding of whole batches on the device (include/gg_jpeg.h): the first stage of the raw-image path.  ``DeviceJpegDecoder(device).decode(files)``
takes a list of JPEG files as ``bytes`` / ``bytearray`` / ``memoryview`` and returns a ``PackedImages``: the packed HWC uint8 RGB batch that ``gg_eval_batch`` and
``gg_aug_batch`` take as ``src`` (``DeviceEvalTransform`` and ``DeviceTrainTransform`` accept it, or the list of file bytes itself), byte for byte what
``PIL.Image.open(f).convert("RGB")`` gives.  The host parses the headers and finds the restart segments (``plan``: no GPU needed), ONE pinned upload moves the tables and
the files, four kernels decode.  Nothing comes back to the host but the per-image status.

``split_bytes`` (``JpegPlan``, ``DeviceJpegDecoder``; 0, the default, is the path above, call for call) turns on the decode with many lanes inside one scan
(include/gg_jscan.h): every restart segment -- the whole scan of a file without restart markers -- is cut into sub-segments of about that many bytes, and
speculate / resolve / write / DC passes take the place of the one-lane-per-segment entropy kernel.  The bytes are the same whatever the value; ``PackedImages.slow``
then counts, per image, the sub-segments no speculative lane reached in the true decoder state.

``progressive=True`` (``JpegPlan``, ``DeviceJpegDecoder``; off by default, and with it off a progressive file is refused as before) turns on the decode of
progressive Huffman files (SOF2; include/gg_jprog.h) next to baseline ones in the same batch: the plan walks every scan of such a file, and the entropy decode runs
in rounds of scans that touch disjoint coefficients (``JpegPlan.scans``, ``JpegPlan.rounds``).  It does not combine with ``split_bytes``."""
import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .._lib import GgError

_EMPTY = (C.c_char * 1)()                 # where a zero-length file points
STATUS_NAMES = {0: "ok", 1: "the entropy-coded data ended early", 2: "an undefined Huffman code was read", 3: "a coefficient index ran past 63"}


class PackedImages(NamedTuple):
    packed: torch.Tensor                  # uint8, flat, on the device: image b is sizes[b][0] x sizes[b][1] x 3 bytes at offsets[b]
    offsets: np.ndarray                   # int64 [B], multiples of 256
    sizes: List[Tuple[int, int]]          # (height, width)
    status: torch.Tensor                  # int32 [B] on the device: 0, or why the image's bytes are all 0
    slow: Optional[torch.Tensor] = None   # int32 [B] on the device, decodes with split_bytes > 0 only: sub-segments that took the resolve pass's slow path
    slots: Optional[np.ndarray] = None    # int32 (N, V) or (N,), DevicePanoramaTransform only: the image of each output slot, -1 for a missing view


def is_file_bytes(x) -> bool:
    return isinstance(x, (bytes, bytearray, memoryview))


def is_file_bytes_list(x) -> bool:
    """A non-empty list / tuple in which every item is file bytes."""
    return isinstance(x, (list, tuple)) and len(x) > 0 and all(is_file_bytes(f) for f in x)


class JpegPlan:
    """The host-side plan of one batch (``gg_jpeg_plan_create``): ``info`` (one ``_lib.JpegInfo`` per file: height, width, components, hs, vs, segments, refusal,
    out_offset, stream_offset), ``stream_bytes`` / ``table_bytes`` / ``output_bytes`` / ``workspace_bytes``.  Needs no GPU.  With ``split_bytes`` > 0 the plan is
    ``gg_jscan_plan_create``'s: the same answers, a sub-segment table in the table block, ``subsegments`` (per image), ``total_subsegments`` and a
    ``workspace_bytes`` that is ``gg_jscan_decode``'s (``base_workspace_bytes`` stays ``gg_jpeg_decode``'s, which takes such a plan too).  With ``progressive`` the plan
    is ``gg_jprog_plan_create``'s: SOF2 files are accepted too, ``scans`` (per image: 1 for a baseline file, 0 for a refused one) and ``rounds`` (the entropy
    launches ``gg_jprog_decode`` needs) are set, and the refusal names are ``gg_jprog_refusal_name``'s."""

    def __init__(self, files: Sequence, split_bytes: int = 0, progressive: bool = False):
        if not is_file_bytes_list(files):
            raise GgError("JpegPlan: files must be a non-empty list of bytes / bytearray / memoryview")
        if len(files) > _lib.JPEG_MAX_B:
            raise GgError(f"JpegPlan: {len(files)} files in one batch, at most {_lib.JPEG_MAX_B}")
        lib = _lib.lib()
        self._views = [np.frombuffer(f, np.uint8) for f in files]          # zero-copy; keeps the buffers alive
        B = len(files)
        self._ptrs = (C.c_void_p * B)(*[v.ctypes.data if v.size else C.addressof(_EMPTY) for v in self._views])
        self._lens = (C.c_int64 * B)(*[v.size for v in self._views])
        self._h = C.c_void_p()
        self.split_bytes = int(split_bytes)
        self.progressive = bool(progressive)
        if self.progressive and self.split_bytes:
            raise GgError("JpegPlan: progressive=True does not combine with split_bytes > 0: progressive scans are not cut into sub-segments")
        if self.progressive:
            _lib.check(lib.gg_jprog_plan_create(self._ptrs, self._lens, B, C.byref(self._h)), "gg_jprog_plan_create")
        elif self.split_bytes:
            _lib.check(lib.gg_jscan_plan_create(self._ptrs, self._lens, B, self.split_bytes, C.byref(self._h)), "gg_jscan_plan_create")
        else:
            _lib.check(lib.gg_jpeg_plan_create(self._ptrs, self._lens, B, C.byref(self._h)), "gg_jpeg_plan_create")
        self.B = B
        self.info = []
        for b in range(B):
            i = _lib.JpegInfo()
            _lib.check(lib.gg_jpeg_plan_info(self._h, b, C.byref(i)), "gg_jpeg_plan_info")
            self.info.append(i)
        self.stream_bytes, self.table_bytes = lib.gg_jpeg_plan_stream_bytes(self._h), lib.gg_jpeg_plan_table_bytes(self._h)
        self.output_bytes, self.workspace_bytes = lib.gg_jpeg_plan_output_bytes(self._h), lib.gg_jpeg_workspace_bytes(self._h)
        self.first_refused = lib.gg_jpeg_plan_first_refused(self._h)
        self.base_workspace_bytes = self.workspace_bytes
        self.subsegments, self.total_subsegments = None, None
        if self.split_bytes:
            self.subsegments = [lib.gg_jscan_plan_subsegments(self._h, b) for b in range(B)]
            self.total_subsegments = lib.gg_jscan_plan_total_subsegments(self._h)
            self.workspace_bytes = lib.gg_jscan_workspace_bytes(self._h)
        self.scans, self.rounds = None, None
        if self.progressive:
            self.scans = [lib.gg_jprog_plan_scans(self._h, b) for b in range(B)]
            self.rounds = lib.gg_jprog_plan_rounds(self._h)
            self.workspace_bytes = lib.gg_jprog_workspace_bytes(self._h)

    def refusal_name(self, b: int) -> str:
        name = _lib.lib().gg_jprog_refusal_name if self.progressive else _lib.lib().gg_jpeg_refusal_name
        return name(self.info[b].refusal).decode()

    def require_accepted(self) -> None:
        if self.first_refused >= 0:
            b = self.first_refused
            raise GgError(f"DeviceJpegDecoder: image {b} is refused: {self.refusal_name(b)}")

    def fill(self, host_ptr: int) -> None:
        """Writes the stream buffer [ table block | files ] into ``stream_bytes`` bytes of host memory."""
        _lib.check(_lib.lib().gg_jpeg_plan_fill(self._h, self._ptrs, host_ptr), "gg_jpeg_plan_fill")

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h:
            _lib.lib().gg_jpeg_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceJpegDecoder:
    """``decode(files) -> PackedImages``.  One pinned staging buffer and one workspace, both the decoder's own and reused from call to call (they grow when a batch
    needs more); the packed output is a fresh tensor per call.  A refused file (progressive, CMYK, ...: include/gg_jpeg.h) raises ``GgError`` naming its index and the
    reason before anything is launched; with ``check=True`` (the default) a file whose entropy data is damaged raises the same way after the decode (one int32 per image
    is read back), with ``check=False`` its image is all zeros and ``status`` says why.  The read-back of ``check=True`` waits for the decode: one host
    synchronisation per batch, also on the transforms' and embedders' paths, which decode with the default; a pipeline that must not wait decodes with
    ``check=False`` itself, hands the ``PackedImages`` on and looks at ``status`` later.  ``split_bytes`` > 0: the decode with many lanes inside one scan
    (``gg_jscan_decode``), for files without restart markers; the same bytes, and ``PackedImages.slow``.  ``progressive=True``: progressive files (SOF2) are decoded
    too (``gg_jprog_decode``), next to baseline ones; not together with ``split_bytes``."""

    def __init__(self, device="cuda", split_bytes: int = 0, progressive: bool = False):
        self.device = torch.device(device)
        self.split_bytes = int(split_bytes)
        self.progressive = bool(progressive)
        if self.progressive and self.split_bytes:
            raise GgError("DeviceJpegDecoder: progressive=True does not combine with split_bytes > 0: progressive scans are not cut into sub-segments")
        self._staging: Optional[torch.Tensor] = None
        self._uploaded: Optional[torch.cuda.Event] = None
        self._workspace: Optional[torch.Tensor] = None

    def decode(self, files: Sequence, check: bool = True) -> PackedImages:
        _lib.require_gpu()
        plan = JpegPlan(list(files) if isinstance(files, (list, tuple)) else [files], self.split_bytes, self.progressive)
        try:
            plan.require_accepted()
            if self._uploaded is not None:
                self._uploaded.synchronize()              # the previous batch's upload has left the staging buffer
            if self._staging is None or self._staging.numel() < plan.stream_bytes:
                self._staging = torch.empty(plan.stream_bytes + plan.stream_bytes // 4, dtype=torch.uint8, pin_memory=True)
            plan.fill(self._staging.data_ptr())
            with torch.cuda.device(self.device):
                stream_buf = self._staging[:plan.stream_bytes].to(self.device, non_blocking=True)
                self._uploaded = torch.cuda.Event()
                self._uploaded.record()
                if self._workspace is None or self._workspace.numel() < plan.workspace_bytes or self._workspace.device != stream_buf.device:
                    self._workspace = None
                    self._workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=self.device)
                packed = torch.empty(max(plan.output_bytes, 1), dtype=torch.uint8, device=self.device)
                status = torch.empty(plan.B, dtype=torch.int32, device=self.device)
                slow = None
                if self.progressive:
                    _lib.check(_lib.lib().gg_jprog_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), packed.data_ptr(), packed.numel(), status.data_ptr(),
                                                          self._workspace.data_ptr(), self._workspace.numel(), _lib.stream()), "gg_jprog_decode")
                elif self.split_bytes:
                    slow = torch.empty(plan.B, dtype=torch.int32, device=self.device)
                    _lib.check(_lib.lib().gg_jscan_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), packed.data_ptr(), packed.numel(), status.data_ptr(),
                                                          slow.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(), _lib.stream()), "gg_jscan_decode")
                else:
                    _lib.check(_lib.lib().gg_jpeg_decode(plan.handle, stream_buf.data_ptr(), stream_buf.numel(), packed.data_ptr(), packed.numel(), status.data_ptr(),
                                                         self._workspace.data_ptr(), self._workspace.numel(), _lib.stream()), "gg_jpeg_decode")
            offsets = np.array([i.out_offset for i in plan.info], np.int64)
            sizes = [(int(i.height), int(i.width)) for i in plan.info]
        finally:
            plan.close()
        if check:
            st = status.cpu().numpy()
            bad = np.nonzero(st)[0]
            if len(bad):
                raise GgError(f"DeviceJpegDecoder: image {int(bad[0])} failed to decode: {STATUS_NAMES.get(int(st[bad[0]]), 'unknown')}")
        return PackedImages(packed, offsets, sizes, status, slow)

    def unpack(self, p: PackedImages) -> List[torch.Tensor]:
        """The images as (H, W, 3) uint8 views of the packed buffer (on the device)."""
        return [p.packed[int(o):int(o) + 3 * h * w].view(h, w, 3) for o, (h, w) in zip(p.offsets, p.sizes)]
