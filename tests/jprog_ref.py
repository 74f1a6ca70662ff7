"""Progressive Huffman JPEG (SOF2) decoding restated in numpy and plain Python, used only as a checker (tests/test_jprog_cpu.py, tests/test_gpu_jprog.py): what
Pillow 12.2 on libjpeg-turbo computes for ``Image.open(f).convert("RGB")`` of a file whose progression is complete, written from T.81 Annex G and libjpeg's
documented arithmetic, independently of csrc/jpeg_progressive.h.  The pixel half (inverse DCT, fancy upsampling, colour) is tests/jpeg_ref.py's.

    parse(data)        -> dict: H, W, ncomp, hs, vs, mcux, mcuy, bpm, quant (per component, as latched at the component's first scan), scans: a list of dicts
                          comps (frame indices), Ss, Se, Ah, Al, dc {component: (counts, values)}, ac, ri, bw, bh, units, segments [(begin, end)], round
    coefficients(data) -> (int16 [blocks, 64] in the baseline decoder's order: MCU by MCU, component by component, zigzag index inside a block; status)
    decode(data)       -> uint8 (H, W, 3)
"""
import numpy as np

from tests import jpeg_ref as J


def parse(data):
    d = bytes(data)
    assert d[:2] == b"\xff\xd8", "no SOI"
    pos, quant, huff, ri = 2, {}, {}, 0
    out = {"scans": []}
    comps, latched = None, {}
    while pos < len(d):
        while pos < len(d) and d[pos] != 0xFF:
            pos += 1
        while pos < len(d) and d[pos] == 0xFF:
            pos += 1
        if pos >= len(d):
            break
        m = d[pos]; pos += 1
        if m == 0xD9:
            break
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xD8:
            continue
        L = d[pos] << 8 | d[pos + 1]
        s = d[pos + 2:pos + L]
        pos += L
        if m == 0xC2:
            assert s[0] == 8
            out["H"], out["W"], out["ncomp"] = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
            if out["ncomp"] == 1:
                out["hs"] = out["vs"] = 1
            else:
                out["hs"], out["vs"] = comps[0][1], comps[0][2]
                assert all(c[1] == 1 and c[2] == 1 for c in comps[1:])
            out["mcux"] = -(-out["W"] // (8 * out["hs"])); out["mcuy"] = -(-out["H"] // (8 * out["vs"]))
            out["bpm"] = out["hs"] * out["vs"] + 2 if out["ncomp"] == 3 else 1
        elif m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                if pq:
                    quant[tq] = np.frombuffer(s[i + 1:i + 129], ">u2").astype(np.int64); i += 129
                else:
                    quant[tq] = np.frombuffer(s[i + 1:i + 65], np.uint8).astype(np.int64); i += 65
        elif m == 0xC4:
            i = 0
            while i < len(s):
                counts = list(s[i + 1:i + 17]); n = sum(counts)
                huff[(s[i] >> 4, s[i] & 15)] = (counts, list(s[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:
            ri = s[0] << 8 | s[1]
        elif m == 0xDA:
            ns = s[0]
            ids = [c[0] for c in comps]
            sc = {"comps": [ids.index(s[1 + 2 * j]) for j in range(ns)], "Ss": s[1 + 2 * ns], "Se": s[2 + 2 * ns], "Ah": s[3 + 2 * ns] >> 4, "Al": s[3 + 2 * ns] & 15,
                  "ri": ri, "dc": {}, "ac": None}
            for j, c in enumerate(sc["comps"]):
                td, ta = s[2 + 2 * j] >> 4, s[2 + 2 * j] & 15
                if sc["Ss"] == 0 and sc["Ah"] == 0:
                    sc["dc"][c] = huff[(0, td)]
                if sc["Ss"] > 0:
                    sc["ac"] = huff[(1, ta)]
                if c not in latched:
                    latched[c] = quant[comps[c][3]].copy()
            if ns == 1:
                c = sc["comps"][0]
                hc, vc = (out["hs"], out["vs"]) if c == 0 else (1, 1)
                sc["bw"], sc["bh"] = -(-(-(-out["W"] // (out["hs"] // hc))) // 8), -(-(-(-out["H"] // (out["vs"] // vc))) // 8)
                sc["units"] = sc["bw"] * sc["bh"]
            else:
                sc["bw"], sc["bh"], sc["units"] = out["mcux"], out["mcuy"], out["mcux"] * out["mcuy"]
            segs, begin, q = [], pos, pos
            while True:
                i = d.find(b"\xff", q)
                if i < 0 or i + 1 >= len(d):
                    segs.append((begin, len(d))); pos = len(d); break
                if d[i + 1] == 0:
                    q = i + 2
                elif d[i + 1] == 0xFF:
                    q = i + 1
                elif 0xD0 <= d[i + 1] <= 0xD7:
                    segs.append((begin, i)); begin = q = i + 2
                else:
                    segs.append((begin, i)); pos = i; break
            sc["segments"] = segs
            out["scans"].append(sc)
    out["quant"] = [latched[c] for c in range(out["ncomp"])]
    last = {}
    for sc in out["scans"]:                               # a scan's round: one more than the latest earlier scan that shares a (component, zigzag index) pair with it
        keys = [(c, k) for c in sc["comps"] for k in range(sc["Ss"], sc["Se"] + 1)]
        sc["round"] = 1 + max([last.get(k, 0) for k in keys])
        for k in keys:
            last[k] = sc["round"]
    return out


def _slot(p, c, by, bx):
    """index of block (by, bx) of component c in the MCU-major coefficient array"""
    hc, vc = (p["hs"], p["vs"]) if c == 0 else (1, 1)
    joff = 0 if c == 0 else p["hs"] * p["vs"] + c - 1
    return ((by // vc) * p["mcux"] + bx // hc) * p["bpm"] + joff + (by % vc) * hc + bx % hc


def _blocks(p, sc, unit0, units):
    """[(component, block index)] of a segment's units in coded order"""
    out = []
    if len(sc["comps"]) > 1:
        b0 = p["hs"] * p["vs"]
        for u in range(unit0, unit0 + units):
            for j in range(p["bpm"]):
                c = 0 if j < b0 else 1 + j - b0
                if c in sc["comps"]:
                    out.append((c, u * p["bpm"] + j))
    else:
        c = sc["comps"][0]
        for u in range(unit0, unit0 + units):
            out.append((c, _slot(p, c, u // sc["bw"], u % sc["bw"])))
    return out


def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def segment(p, sc, seg, unit0, units, coef):
    """Decodes one restart interval of one scan into coef; returns the status (0 / 1 ended early / 2 undefined code / 3 coefficient index past Se)."""
    bits = J._Bits(seg)
    Ss, Se, Ah, Al = sc["Ss"], sc["Se"], sc["Ah"], sc["Al"]
    p1 = 1 << Al
    dct = {c: J._code_table(*t) for c, t in sc["dc"].items()}
    act = J._code_table(*sc["ac"]) if sc["ac"] else None
    pred, eobrun = {}, 0

    def correct(n, k):
        cf = int(coef[n, k])
        if bits.take(1) and (cf & p1) == 0:
            coef[n, k] = _i16(cf + p1 if cf >= 0 else cf - p1)
    try:
        for c, n in _blocks(p, sc, unit0, units):
            if Ss == 0 and Ah == 0:
                s = bits.symbol(dct[c])
                if s > 15:
                    return 2
                pred[c] = pred.get(c, 0) + J._extend(bits.take(s), s)
                coef[n, 0] = _i16(pred[c] << Al)
            elif Ss == 0:
                if bits.take(1):
                    coef[n, 0] = _i16(int(coef[n, 0]) | p1)
            elif Ah == 0:
                if eobrun > 0:
                    eobrun -= 1
                    continue
                k = Ss
                while k <= Se:
                    rs = bits.symbol(act); r, s = rs >> 4, rs & 15
                    if s:
                        k += r
                        v = J._extend(bits.take(s), s)
                        if k > Se:
                            return 3
                        coef[n, k] = _i16(v << Al)
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        eobrun = (1 << r) + bits.take(r) - 1
                        break
            else:
                k = Ss
                if eobrun == 0:
                    while k <= Se:
                        rs = bits.symbol(act); r, s = rs >> 4, rs & 15
                        new = 0
                        if s:
                            v = bits.take(s)
                            if s != 1:
                                return 2
                            new = p1 if v else -p1
                        elif r != 15:
                            eobrun = (1 << r) + bits.take(r)
                            break
                        while k <= Se:
                            if coef[n, k] != 0:
                                correct(n, k)
                            else:
                                r -= 1
                                if r < 0:
                                    break
                            k += 1
                        if s:
                            if k > Se:
                                return 3
                            coef[n, k] = new
                        k += 1
                if eobrun > 0:
                    while k <= Se:
                        if coef[n, k] != 0:
                            correct(n, k)
                        k += 1
                    eobrun -= 1
    except EOFError:
        return 1
    except KeyError:
        return 2
    return 0


def coefficients(data, info=None):
    p = info or parse(data)
    d = bytes(data)
    coef = np.zeros((p["mcux"] * p["mcuy"] * p["bpm"], 64), np.int16)
    status = 0
    for sc in p["scans"]:
        ri = sc["ri"]
        for i, (b, e) in enumerate(sc["segments"]):
            unit0 = i * ri if ri else 0
            units = min(ri, sc["units"] - unit0) if ri else sc["units"]
            if units <= 0:
                break
            status = max(status, segment(p, sc, d[b:e], unit0, units, coef))
    return coef, status


def pixels(p, coef):
    """tests/jpeg_ref.py's decode from the coefficients on: dequantise + inverse DCT, fancy upsampling, Y'CbCr -> RGB"""
    H, W, hs, vs, nc, bpm, mcux, mcuy = p["H"], p["W"], p["hs"], p["vs"], p["ncomp"], p["bpm"], p["mcux"], p["mcuy"]
    coef = coef.reshape(mcuy, mcux, bpm, 64)
    planes, j = [], 0
    for c in range(nc):
        hc, vc = (hs, vs) if c == 0 else (1, 1)
        blk = J.idct_blocks(coef[:, :, j:j + hc * vc].reshape(-1, 64), p["quant"][c]).reshape(mcuy, mcux, vc, hc, 8, 8)
        planes.append(blk.transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * vc * 8, mcux * hc * 8))
        j += hc * vc
    Y = planes[0][:H, :W].astype(np.int64)
    if nc == 1:
        return np.repeat(Y[:, :, None], 3, 2).astype(np.uint8)
    dw, dh = -(-W // hs), -(-H // vs)
    ch = []
    for pl in planes[1:]:
        a = pl[:dh, :dw]
        if hs == 1:
            ch.append(a.astype(np.int64))
        elif dw <= 2:
            ch.append(np.repeat(np.repeat(a.astype(np.int64), vs, 0), 2, 1)[:H, :W])
        else:
            ch.append(J._h2v1(a, W) if vs == 1 else J._h2v2(a, H, W))
    cb, cr = ch[0] - 128, ch[1] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], 2), 0, 255).astype(np.uint8)


def decode(data):
    p = parse(data)
    coef, status = coefficients(data, p)
    assert status == 0, f"entropy decode failed with status {status}"
    return pixels(p, coef)
