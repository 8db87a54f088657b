"""A small FLAC writer in pure Python, for tests: it turns integer PCM into a valid native
FLAC stream whose every coding choice is the caller's (no encoder exists where the tests
run).  STREAMINFO carries the true total and a zero MD5 ("not computed"); frame headers
carry a correct CRC-8 and frames a correct CRC-16.

    stream, offsets = write_stream(pcm, bps, blocks=..., chc=..., sub=...)

``pcm`` is [frames][channels] integers of ``bps`` bits.  ``blocks`` is one block size (the
last frame is then as short as it has to be) or the list of all block sizes.  ``chc`` is the
channel assignment 0-10 (one, or one per frame).  ``sub`` describes a subframe, or is a
function (frame index, channel) -> description; a description is a dict:

    type       "constant" | "verbatim" | "fixed" | "lpc"
    order      FIXED 0-4, LPC 1-32
    precision  LPC coefficient bits (<= 15), shift: LPC shift, coefs: the coefficients (optional)
    method     Rice coding method 0 (4-bit parameters) or 1 (5-bit)
    porder     partition order
    escape     None, "all" or a set of partition indices coded raw; escape_bits: their width
               (None: the narrowest that holds them)
    wasted     wasted bits (the samples must be multiples of 2**wasted)

A frame too short for its description's order and partitions (a short last frame) is written
VERBATIM.

``offsets`` are the true byte offsets of the frames.  CASES names the streams the FLAC tests
share; ``case(name)`` builds one (cached) as (stream, offsets, pcm, bps).
"""
from functools import lru_cache

import numpy as np

BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13,
            16384: 14, 32768: 15}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


def crc8(data: bytes) -> int:
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data: bytes) -> int:
    crc = 0
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[(crc >> 8) ^ b]
    return crc


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def u(self, value: int, bits: int):
        if bits == 0:
            return
        assert 0 <= value < (1 << bits), (value, bits)
        self.acc = (self.acc << bits) | value
        self.n += bits
        if self.n >= 64:
            self._flush()

    def s(self, value: int, bits: int):
        if bits == 0:
            assert value == 0
            return
        assert -(1 << (bits - 1)) <= value < (1 << (bits - 1)), (value, bits)
        self.u(value & ((1 << bits) - 1), bits)

    def unary(self, q: int):
        while q >= 32:
            self.u(0, 32)
            q -= 32
        self.u(1, q + 1)

    def _flush(self):
        whole = self.n // 8
        rest = self.n - whole * 8
        self.out += (self.acc >> rest).to_bytes(whole, "big")
        self.acc &= (1 << rest) - 1
        self.n = rest

    def bytes(self) -> bytes:  # zero-padded to a byte
        if self.n % 8:
            self.u(0, 8 - self.n % 8)
        self._flush()
        return bytes(self.out)


def utf8_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for nbytes in range(2, 8):
        if v < (1 << (5 * nbytes + 1)):
            break
    lead = (0xFF << (8 - nbytes)) & 0xFF
    out = [lead | (v >> (6 * (nbytes - 1)))]
    for k in range(nbytes - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * k)) & 0x3F))
    return bytes(out)


def default_coefs(order: int, precision: int, shift: int, seed: int = 0):
    """A second-order extrapolator in the first taps, small values in the rest (every tap is
    used); all fit ``precision`` bits."""
    rng = np.random.default_rng(1234 + 97 * order + seed)
    lim = 1 << (precision - 1)
    small = max(1, lim >> 5)
    c = [int(x) for x in rng.integers(-small, small + 1, order)]
    one = 1 << shift
    if order == 1:
        c[0] = min(one, lim - 1)
    else:
        c[0], c[1] = min(2 * one, lim - 1), -min(one, lim)
    return [int(np.clip(x, -lim, lim - 1)) or 1 for x in c]


def _residual(w: BitWriter, res, order: int, bs: int, d: dict):
    method, po = d.get("method", 0), d.get("porder", 0)
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    parts = 1 << po
    assert bs % parts == 0 and (bs >> po) >= order, (bs, po, order)
    w.u(method, 2)
    w.u(po, 4)
    escape = d.get("escape")
    k0 = 0
    for pi in range(parts):
        cnt = (bs >> po) - (order if pi == 0 else 0)
        part = res[k0:k0 + cnt]
        k0 += cnt
        if escape == "all" or (escape and pi in escape):
            nb = d.get("escape_bits")
            if nb is None:
                nb = max([0] + [(int(r) if r >= 0 else ~int(r)).bit_length() + 1 for r in part if r != 0])
            w.u(esc, pbits)
            w.u(nb, 5)
            for r in part:
                w.s(int(r), nb)
            continue
        folded = [(2 * int(r)) if r >= 0 else (-2 * int(r) - 1) for r in part]
        mean = sum(folded) // max(len(folded), 1)
        k = d.get("rice")
        if k is None:
            k = min(esc - 1, max(0, mean.bit_length() - 1))
        w.u(k, pbits)
        for v in folded:
            w.unary(v >> k)
            w.u(v & ((1 << k) - 1), k)


def _subframe(w: BitWriter, x, bps: int, d: dict):
    """x: the channel's samples of this frame (Python ints), bps: their width (side: one more)."""
    bs = len(x)
    wasted = d.get("wasted", 0)
    kind = d["type"]
    order = d.get("order", 0)
    if kind in ("fixed", "lpc") and (bs % (1 << d.get("porder", 0)) or (bs >> d.get("porder", 0)) < order):
        kind = "verbatim"  # a (last) frame too short for the description
    code = {"constant": 0, "verbatim": 1}.get(kind)
    if kind == "fixed":
        code = 8 + order
    elif kind == "lpc":
        code = 31 + order
    w.u(0, 1)
    w.u(code, 6)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in x)
        x = [v >> wasted for v in x]
        bps -= wasted
        w.u(1, 1)
        w.unary(wasted - 1)
    else:
        w.u(0, 1)
    if kind == "constant":
        assert all(v == x[0] for v in x)
        w.s(x[0], bps)
    elif kind == "verbatim":
        for v in x:
            w.s(v, bps)
    elif kind == "fixed":
        assert order <= bs
        for v in x[:order]:
            w.s(v, bps)
        co = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}[order]
        res = [x[i] - sum(c * x[i - 1 - j] for j, c in enumerate(co)) for i in range(order, bs)]
        _residual(w, res, order, bs, d)
    else:
        assert 1 <= order <= 32 and order <= bs
        prec, shift = d.get("precision", 12), d.get("shift", 9)
        coefs = d.get("coefs") or default_coefs(order, prec, shift)
        for v in x[:order]:
            w.s(v, bps)
        w.u(prec - 1, 4)
        w.s(shift, 5)
        for c in coefs:
            w.s(c, prec)
        res = [x[i] - (sum(c * x[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, bs)]
        assert all(-(1 << 31) <= r < (1 << 31) for r in res)
        _residual(w, res, order, bs, d)


def _frame(x, bps, number, chc, sub, fi, variable, frame_bits, bs_form, rate):
    """x: [bs][channels] Python ints of one frame."""
    bs = len(x)
    if bs_form == "auto":
        bsc = BS_CODES.get(bs) or (6 if bs <= 256 else 7)
    else:
        bsc = {"8bit": 6, "16bit": 7}[bs_form]
    head = BitWriter()
    head.u(0x3FFE, 14)
    head.u(0, 1)
    head.u(1 if variable else 0, 1)
    head.u(bsc, 4)
    head.u(9 if rate == 44100 else 0, 4)
    head.u(chc, 4)
    head.u(SS_CODES[bps] if frame_bits else 0, 3)
    head.u(0, 1)
    hb = head.bytes() + utf8_number(number)
    if bsc == 6:
        hb += bytes([bs - 1])
    elif bsc == 7:
        hb += (bs - 1).to_bytes(2, "big")
    hb += bytes([crc8(hb)])
    cols = [[row[c] for row in x] for c in range(len(x[0]))]
    widths = [bps] * len(cols)
    if chc == 8:
        cols[1] = [a - b for a, b in zip(cols[0], cols[1])]
        widths[1] += 1
    elif chc == 9:
        cols[0] = [a - b for a, b in zip(cols[0], cols[1])]
        widths[0] += 1
    elif chc == 10:
        left, right = cols
        cols = [[(a + b) >> 1 for a, b in zip(left, right)], [a - b for a, b in zip(left, right)]]
        widths[1] += 1
    else:
        assert chc + 1 == len(cols)
    w = BitWriter()
    for c, col in enumerate(cols):
        _subframe(w, col, widths[c], sub(fi, c) if callable(sub) else sub)
    body = hb + w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def write_stream(pcm, bps, rate=16000, blocks=4096, chc=None, sub=None, variable=False, frame_bits=False,
                 bs_form="auto", total=None, frame_sizes=True):
    """(stream bytes, true frame offsets).  ``total``: the STREAMINFO total (None: the true one);
    ``frame_sizes`` False leaves STREAMINFO's minimum / maximum frame size unknown (0);
    ``frame_bits``: the frame header names the sample size itself instead of pointing to STREAMINFO."""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    n, C = pcm.shape
    rows = pcm.tolist()
    if isinstance(blocks, int):
        sizes = [blocks] * (n // blocks) + ([n % blocks] if n % blocks else [])
    else:
        sizes = list(blocks)
    assert sum(sizes) == n
    if chc is None:
        chc = C - 1
    sub = sub or {"type": "verbatim"}
    frames, at = [], 0
    for fi, bs in enumerate(sizes):
        code = chc[fi] if isinstance(chc, (list, tuple)) else chc
        frames.append(_frame(rows[at:at + bs], bps, at if variable else fi, code, sub, fi, variable, frame_bits,
                             bs_form, rate))
        at += bs
    info = BitWriter()
    info.u(min(sizes[:-1] or sizes), 16)
    info.u(max(sizes), 16)
    info.u(min(map(len, frames)) if frame_sizes else 0, 24)
    info.u(max(map(len, frames)) if frame_sizes else 0, 24)
    info.u(rate, 20)
    info.u(C - 1, 3)
    info.u(bps - 1, 5)
    info.u(n if total is None else total, 36)
    head = b"fLaC" + bytes([0x80, 0, 0, 34]) + info.bytes() + bytes(16)
    offsets, o = [], len(head)
    for f in frames:
        offsets.append(o)
        o += len(f)
    return head + b"".join(frames), offsets


def tone(n, ch, bps, seed=0, amp=0.6):
    """A smooth signal with a little noise: predictors have something to predict."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)[:, None]
    f = rng.uniform(0.002, 0.02, (1, ch))
    full = (1 << (bps - 1)) - 1
    x = amp * full * (0.7 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6, (1, ch))) + 0.3 * np.sin(2 * np.pi * 3.1 * f * t))
    x = x + rng.normal(0, max(1.0, full / 4096), (n, ch))
    return np.clip(np.round(x), -full - 1, full).astype(np.int64)


def false_header(channels=2) -> bytes:
    """A header-shaped byte run with a valid CRC-8: block size code 6 (8-bit form), 44.1 kHz,
    independent channels, the sample size from STREAMINFO, frame number 5."""
    h = bytes([0xFF, 0xF8, 0x69, (channels - 1) << 4, 0x05, 0x1F])
    return h + bytes([crc8(h)])


def _planted():
    """16-bit stereo VERBATIM frames; the samples of the second frame spell a frame header."""
    pcm = tone(3 * 256, 2, 16, seed=5)
    fake = false_header(2)
    words = np.frombuffer(fake + b"\x00", ">i2").astype(np.int64)  # 4 big-endian samples = 8 bytes
    pcm[256 + 10: 256 + 10 + len(words), 0] = words  # frame 1, channel 0: a subframe's samples are byte-aligned
    stream, offsets = write_stream(pcm, 16, rate=44100, blocks=256, sub={"type": "verbatim"})
    assert stream.count(fake) == 1 and stream.find(fake) not in offsets
    return stream, offsets, pcm


def _extremes(bps):
    full = 1 << (bps - 1)
    n = 512
    a = np.where(np.arange(n) % 2 == 0, full - 1, -full)
    pcm = np.stack([a, -1 - a], axis=1).astype(np.int64)
    pcm[100:140, 0] = full - 1
    pcm[100:140, 1] = -full
    return pcm


def _many_small():
    rng = np.random.default_rng(42)
    sizes = [int(s) for s in rng.integers(16, 65, 333)]  # 333 and 666 lanes: the last waves are ragged
    pcm = tone(sum(sizes), 2, 16, seed=9)
    kinds = [{"type": "fixed", "order": 2}, {"type": "lpc", "order": 4, "precision": 10, "shift": 7},
             {"type": "verbatim"}, {"type": "fixed", "order": 0, "method": 1}]
    return dict(pcm=pcm, bps=16, blocks=sizes, variable=True, chc=[(0x1, 8, 9, 10)[f % 4] for f in range(333)],
                sub=lambda f, c: kinds[(f + c) % 4])


def _specs():
    s = {}
    for t in ("constant", "verbatim"):
        pcm = tone(700, 2, 16, seed=1)
        if t == "constant":
            pcm = np.repeat(pcm[::256][:3], 256, axis=0)[:700]
        s[t] = dict(pcm=pcm, bps=16, blocks=256, sub={"type": t})
    for o in range(5):
        s[f"fixed{o}"] = dict(pcm=tone(1000, 2, 16, seed=10 + o), bps=16, blocks=512, sub={"type": "fixed", "order": o, "porder": 2})
    for o in (1, 8, 12, 32):
        s[f"lpc{o}_24bit_p15"] = dict(pcm=tone(1152 + 192, 2, 24, seed=20 + o, amp=0.95), bps=24, blocks=[576, 576, 192],
                                      sub={"type": "lpc", "order": o, "precision": 15, "shift": 12, "porder": 1, "method": 1})
    s["lpc3_p5"] = dict(pcm=tone(600, 1, 16, seed=31), bps=16, blocks=192, sub={"type": "lpc", "order": 3, "precision": 5, "shift": 2})
    for ch in range(1, 9):
        s[f"independent_{ch}ch"] = dict(pcm=tone(400, ch, 16, seed=40 + ch), bps=16, blocks=192, chc=ch - 1,
                                        sub={"type": "fixed", "order": 1})
    for bps in (16, 24):
        for code, name in ((8, "left_side"), (9, "side_right"), (10, "mid_side")):
            pcm = tone(900, 2, bps, seed=50 + code + bps, amp=0.98)
            pcm[:, 1] = -pcm[:, 1]  # the side channel needs its extra bit
            s[f"{name}_{bps}bit"] = dict(pcm=pcm, bps=bps, blocks=576, chc=code, sub={"type": "fixed", "order": 2})
            s[f"{name}_{bps}bit_extremes"] = dict(pcm=_extremes(bps), bps=bps, blocks=256, chc=code,
                                                  sub=lambda f, c: {"type": "verbatim"} if f == 0 else {"type": "fixed", "order": 2, "method": 1})
    s["wasted_bits"] = dict(pcm=tone(800, 2, 16, seed=60, amp=0.1) * 8, bps=16, blocks=256,
                            sub=lambda f, c: {"type": ("verbatim", "fixed", "lpc")[f % 3], "order": 2, "wasted": 3 - c})
    s["wasted_bits_constant"] = dict(pcm=np.full((300, 2), -52 * 4, np.int64), bps=16, blocks=192, chc=8,
                                     sub=lambda f, c: {"type": "constant", "wasted": 2} if c == 0 else {"type": "constant"})
    z = tone(512, 2, 24, seed=61)
    z[256:] = np.cumsum(np.ones((256, 2), np.int64), axis=0)  # a ramp: the FIXED 2 residual is all zeros
    s["escape_0bit"] = dict(pcm=z, bps=24, blocks=256, sub={"type": "fixed", "order": 2, "porder": 1, "escape": {1}})
    s["escape_24bit"] = dict(pcm=tone(512, 2, 24, seed=62), bps=24, blocks=256,
                             sub={"type": "fixed", "order": 1, "porder": 2, "escape": {0, 2}, "escape_bits": 24})
    s["escape_all"] = dict(pcm=tone(384, 1, 16, seed=63), bps=16, blocks=192, sub={"type": "lpc", "order": 2, "escape": "all"})
    s["rice_method1"] = dict(pcm=tone(1024, 2, 24, seed=64, amp=0.99), bps=24, blocks=512,
                             sub=lambda f, c: {"type": "fixed", "order": 0, "method": 1, "porder": 3, "rice": 20 if c else None})
    s["partition_order_max"] = dict(pcm=tone(4096 + 256, 2, 16, seed=65), bps=16, blocks=[4096, 256],
                                    sub=lambda f, c: {"type": "fixed", "order": 1, "porder": 12 if f == 0 else 8})
    for po in range(5):
        s[f"partition_order_{po}"] = dict(pcm=tone(512, 1, 16, seed=66 + po), bps=16, blocks=256,
                                          sub={"type": "lpc", "order": 6, "porder": po, "method": po & 1})
    s["block16_order4"] = dict(pcm=tone(16 * 9, 2, 16, seed=70), bps=16, blocks=16,
                               sub=lambda f, c: {"type": "fixed" if c else "lpc", "order": 4, "porder": f % 3})
    s["blocksize_8bit_form"] = dict(pcm=tone(3 * 192 + 1, 2, 16, seed=71), bps=16, blocks=192, bs_form="8bit",
                                    sub={"type": "fixed", "order": 2})
    s["blocksize_16bit_form"] = dict(pcm=tone(2 * 1000 + 1, 2, 16, seed=72), bps=16, blocks=1000, bs_form="16bit",
                                     sub={"type": "fixed", "order": 3}, frame_sizes=False)
    for bs, code in sorted(BS_CODES.items()):
        if bs <= 4608:
            s[f"blocksize_code_{code}"] = dict(pcm=tone(bs + 17, 1, 16, seed=code), bps=16, blocks=bs, sub={"type": "fixed", "order": 2})
    s["blocksize_codes_13_14"] = dict(pcm=tone(8192 + 16384, 1, 8, seed=73), bps=8, blocks=[8192, 16384],
                                      sub={"type": "fixed", "order": 1}, variable=True)
    s["blocksize_code_15"] = dict(pcm=tone(32768 + 100, 1, 8, seed=74), bps=8, blocks=32768, sub={"type": "fixed", "order": 1})
    for bps in (8, 12, 20):
        s[f"bits_{bps}"] = dict(pcm=tone(700, 2, bps, seed=80 + bps), bps=bps, blocks=256, chc=10,
                                sub={"type": "lpc", "order": 5, "precision": 9, "shift": 6})
        s[f"bits_{bps}_frame_code"] = dict(pcm=tone(500, 1, bps, seed=90 + bps), bps=bps, blocks=192, frame_bits=True,
                                           sub={"type": "fixed", "order": 3})
    for bps in (16, 24):
        s[f"bits_{bps}_frame_code"] = dict(pcm=tone(500, 2, bps, seed=90 + bps), bps=bps, blocks=192, frame_bits=True,
                                           chc=8, sub={"type": "fixed", "order": 1})
    s["extremes_16bit"] = dict(pcm=_extremes(16), bps=16, blocks=128,
                               sub=lambda f, c: {"type": ("verbatim", "fixed", "fixed", "lpc")[f], "order": (0, 4, 1, 2)[f], "method": 1})
    s["extremes_24bit"] = dict(pcm=_extremes(24), bps=24, blocks=128,
                               sub=lambda f, c: {"type": ("verbatim", "fixed", "fixed", "lpc")[f], "order": (0, 4, 1, 2)[f], "method": 1})
    s["variable_blocks"] = dict(pcm=tone(192 + 300 + 4096 + 1, 2, 16, seed=95), bps=16, blocks=[192, 300, 4096, 1],
                                variable=True, chc=[1, 10, 8, 9], sub={"type": "fixed", "order": 0})
    s["many_small_frames"] = _many_small()
    return s


_SPECS = _specs()
CASES = tuple(_SPECS) + ("planted_false_header",)


@lru_cache(maxsize=None)
def case(name):
    """(stream, offsets, pcm int32 [frames][channels], bits per sample)"""
    if name == "planted_false_header":
        stream, offsets, pcm = _planted()
        return stream, offsets, pcm.astype(np.int32), 16
    kw = dict(_SPECS[name])
    pcm, bps = kw.pop("pcm"), kw.pop("bps")
    stream, offsets = write_stream(pcm, bps, **kw)
    pcm = np.asarray(pcm).astype(np.int32)
    pcm.setflags(write=False)
    return stream, offsets, pcm, bps


if __name__ == "__main__":  # python tests/flac_fixture.py DIR: every case as DIR/<name>.flac
    import os
    import sys
    os.makedirs(sys.argv[1], exist_ok=True)
    for _name in CASES:
        with open(os.path.join(sys.argv[1], _name + ".flac"), "wb") as _f:
            _f.write(case(_name)[0])
    print(f"{len(CASES)} streams written to {sys.argv[1]}")
