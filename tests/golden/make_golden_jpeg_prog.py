"""Writes tests/golden/jpeg_prog_pil.npz: progressive JPEG files together with the RGB that Pillow decoded from them (the fixture of include/gg_jprog.h).

    python tests/golden/make_golden_jpeg_prog.py

(a) Pillow's own progressive files (its 10-scan script for colour, 6 scans for grey); (b) files under scan scripts Pillow cannot write, coded by the small progressive
Huffman encoder below from the quantised coefficients of a Pillow baseline file (tests/jpeg_ref.py reads them) with flat Huffman tables (a count is a byte, so the AC
table is 255 nine-bit codes and one ten-bit code; a DC table may only name sizes, so it is 16 five-bit codes); (c) hand-assembled files, one or more per refusal of
gg_jprog_plan_create that gg_jpeg_plan_create does not know.  For (a) and (b) the expected pixels are Pillow's decode of the very file.

Arrays: file_<i>, rgb_<i>, desc; refuse_<i>, refuse_name (gg_jprog_refusal_name), refuse_desc.  Made with Pillow 12.2 (libjpeg-turbo 3.1)."""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import jpeg_ref as J                                # noqa: E402
from tests import jprog_ref as R                               # noqa: E402
from tests.golden.make_golden_jpeg import content, seg        # noqa: E402

SIZES = [(1, 1), (7, 9), (16, 16), (17, 33), (3, 70), (33, 50), (64, 48)]          # (W, H)
MODES = ["4:4:4", "4:2:2", "4:2:0", "grey"]
BAD_SCRIPT, INCOMPLETE, TOO_MANY, DNL = ("bad progressive scan script", "incomplete progression", "more than 64 scans", "DNL marker or a frame height of 0")
JFIF = seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")


def gradient(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.clip(np.stack([20 + 0.8 * xx + 0.4 * yy, 200 - 0.5 * xx, 90 + 0.6 * yy], 2), 0, 255).astype(np.uint8)


def pil_encode(a, mode, quality, **kw):
    im = Image.fromarray(a)
    buf = io.BytesIO()
    if mode == "grey":
        im.convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=mode, **kw)
    return buf.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(bytes(data))).convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- a progressive Huffman encoder (T.81 Annex G)
class Table:
    """A flat canonical code.  ac: 255 codes of nine bits and one of ten; dc: 16 codes of five bits.  ``swap`` permutes the values, for a second table of the same shape."""

    def __init__(self, dc, swap=0):
        self.counts = [0] * 16
        if dc:
            self.counts[4] = 16
            self.vals = [v ^ (swap & 15) for v in range(16)]
        else:
            self.counts[8], self.counts[9] = 255, 1
            self.vals = [v ^ swap for v in range(256)]
        self.code, code, k = {}, 0, 0
        for l in range(1, 17):
            for _ in range(self.counts[l - 1]):
                self.code[self.vals[k]] = (code, l); code += 1; k += 1
            code <<= 1

    def segment(self, tc, th):
        return seg(0xC4, bytes([tc << 4 | th]) + bytes(self.counts) + bytes(self.vals))


class Writer:
    def __init__(self, table):
        self.bits, self.table = [], table

    def put(self, v, n):
        for i in range(n - 1, -1, -1):
            self.bits.append((v >> i) & 1)

    def symbol(self, v):
        self.put(*self.table.code[v])

    def done(self):
        b = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(b), 8):
            v = int("".join(map(str, b[i:i + 8])), 2)
            out.append(v)
            if v == 0xFF:
                out.append(0)
        return bytes(out)


def encode_segment(blocks, Ss, Se, Ah, Al, table):
    """blocks: [(component, the block's 64 coefficients)] of one restart interval in coded order"""
    w = Writer(table)
    state = {"eobrun": 0, "be": []}

    def emit_eobrun():
        n = state["eobrun"]
        if n > 0:
            nb = n.bit_length() - 1
            w.symbol(nb << 4)
            w.put(n & ((1 << nb) - 1), nb)
            state["eobrun"] = 0
        for bit in state["be"]:
            w.put(bit, 1)
        state["be"] = []

    pred = {}
    for c, blk in blocks:
        blk = [int(v) for v in blk]
        if Ss == 0 and Ah == 0:
            t = blk[0] >> Al
            diff = t - pred.get(c, 0)
            pred[c] = t
            nb = abs(diff).bit_length()
            w.symbol(nb)
            w.put(diff if diff >= 0 else (diff - 1) & ((1 << nb) - 1), nb)
        elif Ss == 0:
            w.put((blk[0] >> Al) & 1, 1)
        elif Ah == 0:
            r = 0
            for k in range(Ss, Se + 1):
                a = abs(blk[k]) >> Al
                if a == 0:
                    r += 1
                    continue
                emit_eobrun()
                while r > 15:
                    w.symbol(0xF0); r -= 16
                nb = a.bit_length()
                w.symbol(r << 4 | nb)
                w.put(a if blk[k] > 0 else ~a & ((1 << nb) - 1), nb)
                r = 0
            if r > 0:
                state["eobrun"] += 1
                if state["eobrun"] == 0x7FFF:
                    emit_eobrun()
        else:
            a = [abs(v) >> Al for v in blk]
            eob = max([k for k in range(Ss, Se + 1) if a[k] == 1], default=0)
            r, br = 0, []
            for k in range(Ss, Se + 1):
                if a[k] == 0:
                    r += 1
                    continue
                while r > 15 and k <= eob:
                    emit_eobrun()
                    w.symbol(0xF0); r -= 16
                    for bit in br:
                        w.put(bit, 1)
                    br = []
                if a[k] > 1:
                    br.append(a[k] & 1)
                    continue
                emit_eobrun()
                w.symbol(r << 4 | 1)
                w.put(0 if blk[k] < 0 else 1, 1)
                for bit in br:
                    w.put(bit, 1)
                br, r = [], 0
            if r > 0 or br:
                state["eobrun"] += 1
                state["be"] += br
                if state["eobrun"] == 0x7FFF or len(state["be"]) > 937:
                    emit_eobrun()
    emit_eobrun()
    return w.done()


def frame(base):
    """-> (the frame as tests/jprog_ref.py describes it, the coefficients, the bytes up to and including SOF2) of a Pillow baseline file"""
    p = J.parse(base)
    coef, status = J.coefficients(base, p)
    assert status == 0
    nc = p["ncomp"]
    head = b"\xff\xd8" + JFIF
    for c in range(nc):
        q = p["quant"][c]
        head += seg(0xDB, bytes([0x10 | c]) + b"".join(struct.pack(">H", int(v)) for v in q)) if q.max() > 255 else seg(0xDB, bytes([c]) + bytes(int(v) for v in q))
    comps = [(1, p["hs"] << 4 | p["vs"], 0), (2, 0x11, 1), (3, 0x11, 2)][:nc] if nc == 3 else [(1, 0x11, 0)]
    head += seg(0xC2, struct.pack(">BHHB", 8, p["H"], p["W"], nc) + b"".join(bytes(c) for c in comps))
    return p, coef, head


def restate(base, script, tail=True):
    """The Pillow baseline file ``base`` under ``script``: a list of scans (components, Ss, Se, Ah, Al) or (components, Ss, Se, Ah, Al, options) with options
    ``ri`` (a DRI segment in front of the scan; it stays in force) and ``swap`` (the scan's table is defined anew, permuted by this value)."""
    p, coef, out = frame(base)
    ri = 0
    for sc in script:
        comps, Ss, Se, Ah, Al = sc[:5]
        opt = sc[5] if len(sc) > 5 else {}
        table = Table(Ss == 0, opt.get("swap", 0))
        if not (Ss == 0 and Ah):
            out += table.segment(0 if Ss == 0 else 1, 0)
        if "ri" in opt:
            ri = opt["ri"]
            out += seg(0xDD, struct.pack(">H", ri))
        out += seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, 0]) for c in comps) + bytes([Ss, Se, Ah << 4 | Al]))
        s = {"comps": list(comps)}
        if len(comps) == 1:
            c = comps[0]
            hc, vc = (p["hs"], p["vs"]) if c == 0 else (1, 1)
            s["bw"] = -(-(-(-p["W"] // (p["hs"] // hc))) // 8)
            units = s["bw"] * -(-(-(-p["H"] // (p["vs"] // vc))) // 8)
        else:
            units = p["mcux"] * p["mcuy"]
        step = ri if ri else units
        for n, u0 in enumerate(range(0, units, step)):
            if n:
                out += bytes([0xFF, 0xD0 + (n - 1) % 8])
            out += encode_segment([(c, coef[i]) for c, i in R._blocks(p, s, u0, min(step, units - u0))], Ss, Se, Ah, Al, table)
    return out + (b"\xff\xd9" if tail else b"")


ALL, Y, CB, CR = (0, 1, 2), (0,), (1,), (2,)


def scripts(colour):
    C = [Y, CB, CR] if colour else [Y]
    dc = [(ALL if colour else Y, 0, 0, 0, 0)]
    full = [(c, 1, 63, 0, 0) for c in C]
    s = {}
    s["spectral selection only"] = dc + [(c, a, b, 0, 0) for c in C for a, b in ((1, 5), (6, 20), (21, 63))]
    s["non-interleaved DC scans"] = [(c, 0, 0, 0, 0) for c in C] + full
    s["DC with three refinements"] = [(C[-1] if not colour else ALL, 0, 0, 0, 3)] + full[:1] + [(ALL if colour else Y, 0, 0, 3, 2)] + full[1:] + \
        [(c, 0, 0, 2, 1) for c in C] + [(ALL if colour else Y, 0, 0, 1, 0)]
    s["AC band first coded at Al 3 and refined three times"] = dc + [(c, 1, 63, 0, 3) for c in C] + [(c, 1, 63, 3, 2) for c in C] + \
        [(c, 1, 9, 2, 1) for c in C] + [(c, 10, 63, 2, 1) for c in C] + [(c, 1, 63, 1, 0) for c in C]
    if colour:
        # 25 scans whose rounds differ from their file order: the chroma refinements come before the luma bands are first coded
        s["25 scans out of round order"] = [(CB + CR, 0, 0, 0, 1), (CB, 1, 63, 0, 2), (CB, 1, 63, 2, 1), (CB, 1, 63, 1, 0), (CR, 1, 63, 0, 1), (CR, 1, 63, 1, 0),
                                             (CB + CR, 0, 0, 1, 0), (Y, 0, 0, 0, 0)] + [(Y, a, a + 3, 0, 1) for a in range(1, 61, 4)] + [(Y, 61, 63, 0, 1), (Y, 1, 63, 1, 0)]
        s["DHT and DRI changed between scans"] = [(ALL, 0, 0, 0, 1, {"ri": 2}), (Y, 1, 63, 0, 1, {"ri": 5, "swap": 0x5A}), (CB, 1, 63, 0, 0, {"ri": 0}),
                                                  (CR, 1, 63, 0, 0, {"swap": 0x33, "ri": 1}), (Y, 1, 63, 1, 0, {"swap": 0}), (ALL, 0, 0, 1, 0, {"ri": 3})]
    else:
        s["bands of width 1 (64 scans)"] = dc + [(Y, k, k, 0, 0) for k in range(1, 64)]
        s["DHT and DRI changed between scans"] = [(Y, 0, 0, 0, 1, {"ri": 2}), (Y, 1, 63, 0, 1, {"ri": 5, "swap": 0x5A}), (Y, 1, 63, 1, 0, {"swap": 0, "ri": 0}), (Y, 0, 0, 1, 0, {"ri": 3})]
    return s


# ---------------------------------------------------------------------------------------------------------------- refusals
def refusals(grey_base, colour_base):
    SOI, EOI = b"\xff\xd8", b"\xff\xd9"
    dqt = seg(0xDB, bytes([0]) + bytes([16] * 64)) + seg(0xDB, bytes([1]) + bytes([17] * 64))
    tabs = Table(True).segment(0, 0) + Table(False).segment(1, 0)

    def sof(h=16, w=16):
        return seg(0xC2, struct.pack(">BHHB", 8, h, w, 3) + bytes((1, 0x22, 0)) + bytes((2, 0x11, 1)) + bytes((3, 0x11, 1)))

    def sos(ids, Ss, Se, Ah, Al):
        return seg(0xDA, bytes([len(ids)]) + b"".join(bytes([i, 0]) for i in ids) + bytes([Ss, Se, Ah << 4 | Al]))

    head = SOI + JFIF + dqt + sof() + tabs
    dc = sos((1, 2, 3), 0, 0, 0, 0)
    cases = [
        (BAD_SCRIPT, "an AC scan with two components", head + dc + sos((2, 3), 1, 63, 0, 0) + EOI),
        (BAD_SCRIPT, "Ss 0 with Se 5", head + sos((1,), 0, 5, 0, 0) + EOI),
        (BAD_SCRIPT, "Ss above Se", head + dc + sos((1,), 9, 5, 0, 0) + EOI),
        (BAD_SCRIPT, "Se 64", head + dc + sos((1,), 1, 64, 0, 0) + EOI),
        (BAD_SCRIPT, "a first scan with Ah 1", head + sos((1, 2, 3), 0, 0, 1, 0) + EOI),
        (BAD_SCRIPT, "a refinement whose Ah is not the last Al", head + sos((1, 2, 3), 0, 0, 0, 1) + sos((1, 2, 3), 0, 0, 2, 1) + EOI),
        (BAD_SCRIPT, "a refinement with Al not Ah - 1", head + sos((1, 2, 3), 0, 0, 0, 2) + sos((1, 2, 3), 0, 0, 2, 0) + EOI),
        (BAD_SCRIPT, "an AC scan of a component before its DC scan", head + sos((1,), 0, 0, 0, 0) + sos((2,), 1, 63, 0, 0) + EOI),
        (BAD_SCRIPT, "Al 14", head + sos((1, 2, 3), 0, 0, 0, 14) + EOI),
        (BAD_SCRIPT, "a component id the frame does not have", head + sos((1, 7), 0, 0, 0, 0) + EOI),
        (INCOMPLETE, "the last scan removed, EOI kept", restate(colour_base, scripts(True)["spectral selection only"][:-1])),
        (INCOMPLETE, "cut off between scans", restate(grey_base, scripts(False)["DC with three refinements"][:-1], tail=False)),
        (INCOMPLETE, "DC scans only", restate(colour_base, [(ALL, 0, 0, 0, 0)])),
        (TOO_MANY, "65 scans", restate(grey_base, [(Y, 0, 0, 0, 1)] + [(Y, k, k, 0, 0) for k in range(1, 64)] + [(Y, 0, 0, 1, 0)])),
        (DNL, "a DNL segment behind the scans", restate(grey_base, scripts(False)["non-interleaved DC scans"], tail=False) + seg(0xDC, b"\0\x10") + EOI),
        (DNL, "frame height 0", SOI + JFIF + dqt + sof(h=0) + tabs + dc + EOI),
    ]
    return cases


def main():
    rng = np.random.default_rng(20261020)
    kinds, quals = ["smooth", "noise", "checker"], [30, 75, 95, 100]
    files, desc = [], []
    n = 0
    for (w, h) in SIZES:                                      # (a) every size in every sampling, content and quality rotating
        for mode in MODES:
            kind, q = kinds[n % 3], quals[n % 4]; n += 1
            files.append(pil_encode(content(kind, w, h, rng), mode, q, progressive=True)); desc.append(f"{w}x{h} {mode} {kind} q{q} pillow")
    for mode in MODES:
        files.append(pil_encode(content("noise", 33, 50, rng), mode, 75, progressive=True, restart_marker_blocks=3)); desc.append(f"33x50 {mode} noise q75 pillow restart_marker_blocks")
        files.append(pil_encode(content("smooth", 64, 48, rng), mode, 95, progressive=True, restart_marker_rows=1)); desc.append(f"64x48 {mode} smooth q95 pillow restart_marker_rows")
        files.append(pil_encode(gradient(64, 48), mode, 75, progressive=True, restart_marker_rows=1)); desc.append(f"64x48 {mode} gradient q75 pillow restart_marker_rows")
        files.append(pil_encode(gradient(33, 50), mode, 30, progressive=True)); desc.append(f"33x50 {mode} gradient q30 pillow")
        files.append(pil_encode(content("checker", 17, 33, rng), mode, 100, progressive=True)); desc.append(f"17x33 {mode} checker q100 pillow")
    files.append(pil_encode(content("smooth", 33, 50, rng), "4:2:0", 75, progressive=True, comment=b"a comment segment", exif=b"Exif\0\0MM\0*\0\0\0\x08\0\0\0\0\0\0"))
    desc.append("33x50 4:2:0 smooth q75 pillow comment exif")
    bases = {"4:2:0": pil_encode(content("noise", 33, 50, rng), "4:2:0", 90), "4:2:2": pil_encode(content("smooth", 17, 33, rng), "4:2:2", 95),
             "4:4:4": pil_encode(content("noise", 7, 9, rng), "4:4:4", 75), "grey": pil_encode(content("noise", 17, 33, rng), "grey", 90)}
    for mode, base in bases.items():                          # (b) scan scripts Pillow cannot write
        for name, script in scripts(mode != "grey").items():
            if mode in ("4:2:2", "4:4:4") and name not in ("non-interleaved DC scans", "DHT and DRI changed between scans", "25 scans out of round order"):
                continue
            data = restate(base, script)
            assert np.array_equal(pil_rgb(data), pil_rgb(base)), (mode, name)       # the same coefficients: Pillow decodes the restated file to the baseline file's pixels
            p = J.parse(base)
            files.append(data); desc.append(f"{p['W']}x{p['H']} {mode} script: {name}")
    out = {}
    for i, f in enumerate(files):
        rgb = pil_rgb(f)
        out[f"file_{i}"], out[f"rgb_{i}"] = np.frombuffer(f, np.uint8), rgb
        assert np.array_equal(R.decode(f), rgb), desc[i]
    out["desc"] = np.array(desc)
    ref = refusals(bases["grey"], bases["4:2:0"])
    for i, (_, _, data) in enumerate(ref):
        out[f"refuse_{i}"] = np.frombuffer(data, np.uint8)
    out["refuse_name"] = np.array([r[0] for r in ref])
    out["refuse_desc"] = np.array([r[1] for r in ref])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_prog_pil.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(files)} files, {len(ref)} refusals, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
