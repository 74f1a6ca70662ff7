"""The decode of one JPEG segment with many lanes (include/gg_jscan.h) restated in plain Python, used only as a checker (tests/test_jscan_cpu.py,
tests/golden/make_golden_jpeg_split.py): the cut into sub-segments, the speculative lanes, and the walk that resolves them, written over ABSOLUTE data-bit positions
of the un-stuffed segment -- independently of csrc/jpeg_entropy.h, which keeps positions relative to a lane's first byte and reads stuffed bytes.  It answers what the
scheme's bookkeeping must give: the status (the sequential decoder's, tests/jpeg_ref.py), the sub-segment count and how many sub-segments no speculative lane
reached in the true state (the slow path).  A symbol step is a pure function of (bit position, block in the MCU, zigzag index); the steps are memoised, so the
many lanes that walk the same states cost one dictionary look-up per step.

    cut(seg, split)                                   -> [(first raw byte, data bytes in front)], data bytes of the segment
    run(seg, mcus, ncomp, blocks, dc, ac, split)      -> dict: status, slow, nsub, synced (sub-segments a speculative lane reached in the true state)
"""
from tests import jpeg_ref as J

OK, ENDED_EARLY, BAD_CODE, COEF_INDEX = 0, 1, 2, 3


def cut(seg, split):
    """A cut lies right behind a data byte, at least `split` raw bytes behind the cut in front and at least `split` in front of the end."""
    cuts, i, d, n, nxt = [(0, 0)], 0, 0, len(seg), split
    while i < n:
        if seg[i] != 0xFF:
            i += 1
        else:
            k = i + 1
            while k < n and seg[k] == 0xFF:
                k += 1
            if k < n and seg[k] == 0:
                i = k + 1
            else:
                break
        d += 1
        if i >= nxt and n - i >= split:
            cuts.append((i, d)); nxt = i + split
    return cuts, d


class _Stepper:
    def __init__(self, seg, ncomp, blocks, dc, ac):
        self.bits = J._Bits(seg).bits
        self.total = len(self.bits)
        self.comp = [c for c in range(ncomp) for _ in range(blocks[c])]
        self.bpm = len(self.comp)
        self.dc = [J._code_table(*t) for t in dc]
        self.ac = [J._code_table(*t) for t in ac]
        self.memo = {}

    def step(self, pos, jm, k):
        """-> (status, pos', jm', k', blocks completed)"""
        key = (pos, jm, k)
        r = self.memo.get(key)
        if r is None:
            r = self.memo[key] = self._step(pos, jm, k)
        return r

    def _step(self, pos, jm, k):
        table = (self.dc if k == 0 else self.ac)[self.comp[jm]]
        peek = self.bits[pos:pos + 16].ljust(16, "0")                        # behind the data the reader sees zeros
        sym = None
        for l in range(1, 17):
            sym = table.get((l, int(peek[:l], 2)))
            if sym is not None:
                break
        if sym is None or (k == 0 and sym > 15):
            return (BAD_CODE, pos, jm, k, 0)
        s, r = sym & 15, (0 if k == 0 else sym >> 4)
        pos += l + s
        if pos > self.total:
            return (ENDED_EARLY, pos, jm, k, 0)
        if k == 0:
            k = 1
        elif s == 0:
            k = k + 16 if r == 15 else 64
        else:
            k += r
            if k > 63:
                return (COEF_INDEX, pos, jm, k, 0)
            k += 1
        if k >= 64:
            return (OK, pos, (jm + 1) % self.bpm, 0, 1)
        return (OK, pos, jm, k, 0)

    def scan(self, pos, jm, k, b1, b2, recover=False):
        """From a step start at pos: -> (state at b1 or None, blocks before it, state at b2 or None, blocks between, error behind b1 or 0, blocks between b1 and it).
        A state is (bits behind the boundary, jm, k); b1 None: counting starts at once; b2 None: the run ends with an error."""
        s1 = s2 = None
        c01 = cnt = err = err_cnt = 0
        in2 = b1 is None
        while True:
            if not in2 and pos >= b1:
                s1, c01, cnt, in2 = (pos - b1, jm, k), cnt, 0, True
            if in2 and b2 is not None and pos >= b2:
                s2 = (pos - b2, jm, k)
                break
            st, pos, jm, k, done = self.step(pos, jm, k)
            if st == COEF_INDEX and recover and not in2:                     # a guessing lane in front of its first boundary: take the block as ended and go on
                st, jm, k = OK, (jm + 1) % self.bpm, 0
            if st:
                if in2:
                    err, err_cnt = st, cnt
                break
            cnt += done
        return s1, c01, s2, cnt, err, err_cnt


def run(seg, mcus, ncomp, blocks, dc, ac, split):
    cuts, dtotal = cut(seg, split)
    n, nb = len(cuts), mcus * sum(blocks[:ncomp])
    S = _Stepper(seg, ncomp, blocks, dc, ac)
    bnd = [8 * d for _, d in cuts] + [None]                                 # behind the last sub-segment there is no boundary
    if n == 1:                                                              # one lane decodes the whole segment: nothing to resolve
        coef_status = _sequential(S, nb)
        return dict(status=coef_status, slow=0, nsub=1, synced=0)
    lanes = {}
    for j in range(n - 1):
        for ph in range(S.bpm if j else 1):
            lanes[(j, ph)] = S.scan(bnd[j], ph, 0, bnd[j + 1], bnd[j + 2], recover=j > 0)
    state, C, status, slow, synced = (0, 0, 0), 0, None, 0, 0
    for j in range(n):
        hit = None
        if j == 0:
            s1, c01 = lanes[(0, 0)][:2]
            if s1 is not None:
                hit = (s1, c01, 0, 0)
        else:
            for ph in range(S.bpm if j > 1 else 1):
                s1, _, s2, c12, err, err_cnt = lanes[(j - 1, ph)]
                if s1 == state:
                    hit = (s2, c12, err, err_cnt)
                    break
        if hit is None:
            slow += 1
            _, _, s2, c12, err, err_cnt = S.scan(bnd[j] + state[0], state[1], state[2], None, bnd[j + 1])
            hit = (s2, c12, err, err_cnt)
        else:
            synced += 1
        nxt, cnt, err, err_cnt = hit
        if err:
            status = OK if C + err_cnt >= nb else err
            break
        C += cnt
        if C >= nb:
            status = OK
            break
        state = nxt
    return dict(status=ENDED_EARLY if status is None else status, slow=slow, nsub=n, synced=synced)


def _sequential(S, nb):
    pos, jm, k, C = 0, 0, 0, 0
    while C < nb:
        st, pos, jm, k, done = S.step(pos, jm, k)
        if st:
            return st
        C += done
    return OK
