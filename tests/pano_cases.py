"""Shared by tests/test_pano_cpu.py, tests/test_gpu_pano.py and tests/test_gpu_guards_pano.py: the cases of tests/golden/pano_pil.npz and the host tables of one
gg_pano_batch call (include/gg_pano.h) through the ABI.  A plain module: no fixtures, no pytest settings."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def load_cases():
    """[{i, src, rs, target, u8, plain, norm}] of the fixture (read-only arrays but for the sources, which torch.from_numpy wants writable)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "pano_pil.npz"))
    assert tuple(np.float32(v) for v in MEAN) == tuple(g["mean"]) and tuple(np.float32(v) for v in STD) == tuple(g["std"])
    cases = []
    for i, (h, w, rs, ht, wt) in enumerate(g["cases"]):
        c = dict(i=i, src=g[f"src{i}"], rs=int(rs), target=(int(ht), int(wt)), u8=g[f"u8_{i}"], plain=g[f"plain{i}"], norm=g[f"norm{i}"])
        assert c["src"].shape == (h, w, 3)
        for k in ("u8", "plain", "norm"):
            c[k].setflags(write=False)
        cases.append(c)
    return cases


class PanoTables:
    """Host tables of one call (kept alive next to the args that point into them): images packed `lead` bytes into the buffer with `gap` bytes between them."""

    def __init__(self, L, srcs, slots, rs, target, normalize=True, gap=0, lead=0, **kw):
        self.srcs = srcs
        starts, at = [], lead
        for s in srcs:
            starts.append(at)
            at += s.size + gap
        self.host = np.full(max(at, 1), 0xA5, np.uint8)
        for s, o in zip(srcs, starts):
            self.host[o:o + s.size] = s.reshape(-1)
        self.offsets = np.array(starts, np.int64)
        self.heights, self.widths = np.array([s.shape[0] for s in srcs], np.int32), np.array([s.shape[1] for s in srcs], np.int32)
        self.slots = np.array(slots, np.int32).reshape(-1)                     # a copy: the guard tests wipe it after the call
        a = L.PanoArgs()
        a.src_bytes = self.host.size
        a.offsets, a.heights, a.widths = self.offsets.ctypes.data, self.heights.ctypes.data, self.widths.ctypes.data
        a.num_images, a.num_slots, a.slot_image = len(srcs), self.slots.size, self.slots.ctypes.data
        a.resize, a.Ht, a.Wt, a.normalize = rs, target[0], target[1], int(normalize)
        a.mean, a.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        for k, v in kw.items():
            setattr(a, k, v)
        self.args = a

    def resized_sizes(self, L):
        out = []
        for h, w in zip(self.heights, self.widths):
            hr, wr = C.c_int(), C.c_int()
            L.check(L.lib().gg_pano_resized_size(int(h), int(w), self.args.resize, C.byref(hr), C.byref(wr)), "gg_pano_resized_size")
            out.append((hr.value, wr.value))
        return out


def pano_batch(L, srcs, slots, rs, target, normalize=True, gap=0, lead=0, ws_fill=0, want_u8=True, u8_gap=0):
    """One gg_pano_batch call on the GPU -> (dst (S, 3, Ht, Wt) numpy, [resized uint8 (Hr, Wr, 3) numpy per image] or None).  The source must come back unchanged,
    and of the uint8 output only the images' own bytes may be written."""
    import torch
    t = PanoTables(L, srcs, slots, rs, target, normalize, gap, lead)
    a = t.args
    packed = torch.from_numpy(t.host).cuda()
    need = L.lib().gg_pano_workspace_bytes(C.byref(a))
    assert need >= 0, L.lib().gg_last_error()
    ws = torch.full((max(need, 8),), ws_fill, dtype=torch.uint8, device="cuda")
    dst = torch.full((t.slots.size, 3, target[0], target[1]), float("nan"), device="cuda")
    a.src, a.dst, a.workspace, a.workspace_bytes = packed.data_ptr(), dst.data_ptr(), ws.data_ptr(), need
    sizes = t.resized_sizes(L)
    if want_u8:
        u8_offsets, at = [], u8_gap
        for hr, wr in sizes:
            u8_offsets.append(at)
            at += 3 * hr * wr + u8_gap
        u8_offsets = np.array(u8_offsets, np.int64)
        u8 = torch.full((max(at, 1),), 0x5A, dtype=torch.uint8, device="cuda")
        a.dst_u8, a.u8_offsets, a.dst_u8_bytes = u8.data_ptr(), u8_offsets.ctypes.data, u8.numel()
    L.check(L.lib().gg_pano_batch(C.byref(a), L.stream()), "gg_pano_batch")
    torch.cuda.synchronize()
    assert torch.equal(packed.cpu(), torch.from_numpy(t.host))
    if not want_u8:
        return dst.cpu().numpy(), None
    flat = u8.cpu().numpy()
    outs, mask = [], np.ones(flat.size, bool)
    for o, (hr, wr) in zip(u8_offsets, sizes):
        outs.append(flat[o:o + 3 * hr * wr].reshape(hr, wr, 3).copy())
        mask[o:o + 3 * hr * wr] = False
    assert (flat[mask] == 0x5A).all()
    return dst.cpu().numpy(), outs
