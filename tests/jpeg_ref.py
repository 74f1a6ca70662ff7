"""Baseline JPEG decoding restated in numpy, used only as a checker (tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py): what Pillow 12.2 on libjpeg defaults
(JDCT_ISLOW, fancy upsampling) computes for ``Image.open(f).convert("RGB")``, written from the JPEG standard and libjpeg's documented arithmetic, independently of
csrc/jpeg.hip.  Plain Python entropy decoding: meant for the small fixture images.

    parse(data)        -> dict: H, W, ncomp, hs, vs, ri, quant (per component, zigzag order), dc / ac (per component: (counts[16], values)), segments [(begin, end)]
    coefficients(data) -> (int16 [blocks, 64] in coded order: MCU by MCU, component by component, zigzag index inside a block; status 0 / 1 ended early /
                          2 undefined code / 3 coefficient index past 63)
    decode(data)       -> uint8 (H, W, 3)
"""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def parse(data):
    d = bytes(data)
    assert d[:2] == b"\xff\xd8", "no SOI"
    pos, quant, huff, out = 2, {}, {}, {"ri": 0}
    while True:
        assert d[pos] == 0xFF, "marker expected"
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]; pos += 1
        L = d[pos] << 8 | d[pos + 1]
        s = d[pos + 2:pos + L]
        pos += L
        if m in (0xC0, 0xC1):
            assert s[0] == 8
            out["H"], out["W"], out["ncomp"] = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            comps = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
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
            out["ri"] = s[0] << 8 | s[1]
        elif m == 0xDA:
            assert s[0] == out["ncomp"]
            sel = [(s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15) for c in range(s[0])]
            break
    if out["ncomp"] == 1:
        out["hs"] = out["vs"] = 1
    else:
        out["hs"], out["vs"] = comps[0][1], comps[0][2]
        assert all(c[1] == 1 and c[2] == 1 for c in comps[1:])
    out["quant"] = [quant[c[3]] for c in comps]
    out["dc"] = [huff[(0, t[0])] for t in sel]
    out["ac"] = [huff[(1, t[1])] for t in sel]
    segs, begin, q = [], pos, pos
    while True:
        i = d.find(b"\xff", q)
        if i < 0 or i + 1 >= len(d):
            segs.append((begin, len(d))); break
        if d[i + 1] == 0:
            q = i + 2
        elif d[i + 1] == 0xFF:
            q = i + 1
        elif 0xD0 <= d[i + 1] <= 0xD7:
            segs.append((begin, i)); begin = q = i + 2
        else:
            segs.append((begin, i)); break
    out["segments"] = segs
    out["mcux"] = -(-out["W"] // (8 * out["hs"])); out["mcuy"] = -(-out["H"] // (8 * out["vs"]))
    out["bpm"] = out["hs"] * out["vs"] + 2 if out["ncomp"] == 3 else 1
    return out


def _code_table(counts, vals):
    """(length, code) -> value of the canonical code"""
    t, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            t[(l, code)] = vals[k]; code += 1; k += 1
        code <<= 1
    return t


class _Bits:
    def __init__(self, seg):
        out, i, n = bytearray(), 0, len(seg)
        while i < n:                                      # un-stuff; FF (or a run of them) followed by anything but 00, or reaching the end, ends the data
            v = seg[i]
            if v == 0xFF:
                k = i + 1
                while k < n and seg[k] == 0xFF:           # FF bytes in a row count as one (libjpeg's reader)
                    k += 1
                if k < n and seg[k] == 0:
                    out.append(0xFF); i = k + 1
                else:
                    break
            else:
                out.append(v); i += 1
        self.bits = "".join(f"{v:08b}" for v in out)
        self.pos = 0

    def take(self, n):
        v = self.bits[self.pos:self.pos + n]
        self.pos += n
        if len(v) < n:
            raise EOFError
        return int(v, 2) if n else 0

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = code << 1 | self.take(1)
            if (l, code) in table:
                return table[(l, code)]
        raise KeyError


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def segment_coefficients(seg, mcus, ncomp, blocks, dc, ac, coef):
    """Decodes one segment into coef [mcus * sum(blocks), 64] (zeroed by the caller); returns the status."""
    bits = _Bits(seg)
    dct, act = [_code_table(*t) for t in dc], [_code_table(*t) for t in ac]
    pred, n = [0] * ncomp, 0
    try:
        for _ in range(mcus):
            for c in range(ncomp):
                for _ in range(blocks[c]):
                    s = bits.symbol(dct[c])
                    if s > 15:
                        return 2
                    pred[c] += _extend(bits.take(s), s)
                    coef[n, 0] = np.int16(np.int64(pred[c]).astype(np.int16))
                    k = 1
                    while k < 64:
                        rs = bits.symbol(act[c]); r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        v = _extend(bits.take(s), s)
                        if k > 63:
                            return 3
                        coef[n, k] = v
                        k += 1
                    n += 1
    except EOFError:
        return 1
    except KeyError:
        # an undefined code whose bits run past the end of the data is an early end first
        return 2
    return 0


def coefficients(data, info=None):
    p = info or parse(data)
    d = bytes(data)
    total = p["mcux"] * p["mcuy"]
    blocks = [p["hs"] * p["vs"], 1, 1][:p["ncomp"]]
    coef = np.zeros((total * p["bpm"], 64), np.int16)
    status, ri = 0, p["ri"]
    for i, (b, e) in enumerate(p["segments"]):
        mcu0 = i * ri if ri else 0
        mcus = min(ri, total - mcu0) if ri else total
        if mcus <= 0:
            break
        status = max(status, segment_coefficients(d[b:e], mcus, p["ncomp"], blocks, p["dc"], p["ac"], coef[mcu0 * p["bpm"]:(mcu0 + mcus) * p["bpm"]]))
    return coef, status


def _pass(v, shift):
    """libjpeg jidctint.c, one 8-point pass along axis 0 of int64 v (values stay inside int32 for real files)"""
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * -15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (v[0] + v[4]) << 13
    tmp1 = (v[0] - v[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = (1 << (shift - 1))
    return np.stack([(tmp10 + tmp3 + r) >> shift, (tmp11 + tmp2 + r) >> shift, (tmp12 + tmp1 + r) >> shift, (tmp13 + tmp0 + r) >> shift,
                     (tmp13 - tmp0 + r) >> shift, (tmp12 - tmp1 + r) >> shift, (tmp11 - tmp2 + r) >> shift, (tmp10 - tmp3 + r) >> shift])


_RANGE = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, np.int64), np.arange(0, 128)]).astype(np.uint8)


def idct_blocks(coef, quant):
    """coef [n, 64] zigzag order, quant [64] zigzag order -> uint8 [n, 8, 8]"""
    nat = np.zeros((coef.shape[0], 64), np.int64)
    nat[:, ZIGZAG] = coef.astype(np.int64) * quant[None, :]
    v = nat.reshape(-1, 8, 8).transpose(1, 2, 0)          # [row, col, n]: pass 1 runs down the columns
    v = _pass(v, 11)
    v = _pass(v.transpose(1, 0, 2), 18)                   # [col', row, n] -> pass 2 along the rows; result [col, row, n]
    return _RANGE[(v & 1023)].transpose(2, 1, 0)


def _h2v1(a, W):
    dw = a.shape[1]
    a = a.astype(np.int64)
    left = np.concatenate([a[:, :1], a[:, :-1]], 1); right = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    out = np.empty((a.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0] = a[:, 0]; out[:, -1] = a[:, -1]
    return out[:, :W]


def _h2v2(a, H, W):
    dh, dw = a.shape
    a = a.astype(np.int64)
    up = np.concatenate([a[:1], a[:-1]], 0); down = np.concatenate([a[1:], a[-1:]], 0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for v, nb in ((0, up), (1, down)):
        s = 3 * a + nb
        left = np.concatenate([s[:, :1], s[:, :-1]], 1); right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        row = np.empty((dh, 2 * dw), np.int64)
        row[:, 0::2] = (3 * s + left + 8) >> 4
        row[:, 1::2] = (3 * s + right + 7) >> 4
        row[:, 0] = (4 * s[:, 0] + 8) >> 4; row[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[v::2] = row
    return out[:H, :W]


def decode(data):
    p = parse(data)
    coef, status = coefficients(data, p)
    assert status == 0, f"entropy decode failed with status {status}"
    H, W, hs, vs, nc, bpm, mcux, mcuy = p["H"], p["W"], p["hs"], p["vs"], p["ncomp"], p["bpm"], p["mcux"], p["mcuy"]
    coef = coef.reshape(mcuy, mcux, bpm, 64)
    planes, j = [], 0
    for c in range(nc):
        hc, vc = (hs, vs) if c == 0 else (1, 1)
        blk = idct_blocks(coef[:, :, j:j + hc * vc].reshape(-1, 64), p["quant"][c]).reshape(mcuy, mcux, vc, hc, 8, 8)
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
        elif dw <= 2:                                     # libjpeg takes the fancy forms only for downsampled widths above 2: plain replication here
            ch.append(np.repeat(np.repeat(a.astype(np.int64), vs, 0), 2, 1)[:H, :W])
        else:
            ch.append(_h2v1(a, W) if vs == 1 else _h2v2(a, H, W))
    cb, cr = ch[0] - 128, ch[1] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], 2), 0, 255).astype(np.uint8)
