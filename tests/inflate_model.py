"""The BGZF reader of DESIGN.md 7.13 in plain Python over the standard library: a strict inflater of RFC 1951 that reads bit by bit, in the
order a sequential reader does, and names the first thing that is wrong (the MONI_INF_* reasons of include/moni_hip.h); a bit writer that
makes DEFLATE blocks from given code lengths and tokens; a bgzip over zlib.  No project code."""
import struct
import zlib

from tests import bgzf_model as bm

OK, HEADER, BTYPE, STORED_LEN, CODE_LENGTHS, BAD_SYMBOL, DISTANCE, OVERRUN, TRUNCATED, TRAILING, ISIZE, CRC = range(12)
MAX_OUT = 65536
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Bad(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


class Bits:
    def __init__(self, data: bytes):
        self.d, self.pos = data, 0          # pos in bits

    def bit(self) -> int:
        if self.pos >= 8 * len(self.d):
            raise Bad(TRUNCATED)
        b = (self.d[self.pos >> 3] >> (self.pos & 7)) & 1
        self.pos += 1
        return b

    def take(self, n: int) -> int:
        v = 0
        for i in range(n):
            v |= self.bit() << i
        return v


def canonical(lengths):
    """(codes per length, symbols in code order) of a set of lengths, or None where zlib would refuse it: over-subscribed, or incomplete with
    anything but no code at all or a single code of length 1"""
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    left, maxl = 1, 0
    for l in range(1, 16):
        left = (left << 1) - cnt[l]
        if left < 0:
            return None
        if cnt[l]:
            maxl = l
    if left > 0 and maxl > 1:
        return None
    syms = [s for l in range(1, 16) for s, x in enumerate(lengths) if x == l]
    return cnt, syms


def decode(B: Bits, code):
    cnt, syms = code
    c = first = index = 0
    for l in range(1, 16):
        c |= B.bit()
        if c - cnt[l] < first:
            return syms[index + (c - first)]
        index += cnt[l]
        first = (first + cnt[l]) << 1
        c <<= 1
    raise Bad(BAD_SYMBOL)


def inflate_payload(payload: bytes, isize: int, trace=None):
    """-> (bytes, [BTYPE of every block seen], reason).  The bytes are what was made before the reason, all of them where it is OK.
    trace: a list that takes, per block, [the offset of its first byte, the lowest offset a match of it reads, its largest distance]."""
    B, out, types = Bits(payload), bytearray(), []
    cap = min(isize, MAX_OUT)
    try:
        last = 0
        while not last:
            last = B.bit()
            t = B.take(2)
            if t == 3:
                raise Bad(BTYPE)
            types.append(t)
            blk = [len(out), len(out), 0]
            if trace is not None:
                trace.append(blk)
            if t == 0:
                B.pos = (B.pos + 7) & ~7
                n, nn = B.take(16), B.take(16)
                if (n ^ 0xFFFF) != nn:
                    raise Bad(STORED_LEN)
                at = B.pos >> 3
                for k in range(n):
                    if at + k >= len(payload):
                        raise Bad(TRUNCATED)
                    if len(out) >= cap:
                        raise Bad(OVERRUN)
                    out.append(payload[at + k])
                B.pos += 8 * n
                continue
            if t == 1:
                ll, dl = FIXED_LIT, FIXED_DIST
            else:
                nlit, ndist, ncl = B.take(5) + 257, B.take(5) + 1, B.take(4) + 4
                if nlit > 286 or ndist > 30:
                    raise Bad(CODE_LENGTHS)
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = B.take(3)
                if sum(1 << (7 - l) for l in cl if l) != 128:
                    raise Bad(CODE_LENGTHS)
                cc = canonical(cl)
                lens = []
                while len(lens) < nlit + ndist:
                    s = decode(B, cc)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise Bad(CODE_LENGTHS)
                        prev, rep = lens[-1], 3 + B.take(2)
                    elif s == 17:
                        prev, rep = 0, 3 + B.take(3)
                    else:
                        prev, rep = 0, 11 + B.take(7)
                    if len(lens) + rep > nlit + ndist:
                        raise Bad(CODE_LENGTHS)
                    lens += [prev] * rep
                ll, dl = lens[:nlit], lens[nlit:]
                if not ll[256]:
                    raise Bad(CODE_LENGTHS)
            lc, dc = canonical(ll), canonical(dl)
            if lc is None or dc is None:
                raise Bad(CODE_LENGTHS)
            while True:
                s = decode(B, lc)
                if s < 256:
                    if len(out) >= cap:
                        raise Bad(OVERRUN)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise Bad(BAD_SYMBOL)
                n = LEN_BASE[s - 257] + B.take(LEN_EXTRA[s - 257])
                d = decode(B, dc)
                if d >= 30:
                    raise Bad(BAD_SYMBOL)
                dist = DIST_BASE[d] + B.take(DIST_EXTRA[d])
                if dist > len(out):
                    raise Bad(DISTANCE)
                if n > cap - len(out):
                    raise Bad(OVERRUN)
                blk[1], blk[2] = min(blk[1], len(out) - dist), max(blk[2], dist)
                for _ in range(n):
                    out.append(out[-dist])
        if (B.pos + 7) // 8 != len(payload):
            raise Bad(TRAILING)
        if len(out) != isize:
            raise Bad(ISIZE)
    except Bad as e:
        return bytes(out), types, e.reason
    return bytes(out), types, OK


def member_at(data: bytes, at: int):
    """-> ('ok', total, payload offset) | ('short',) | ('bad',): the member that starts at data[at]"""
    if len(data) - at < 12:
        return ("short",)
    if data[at:at + 4] != b"\x1f\x8b\x08\x04":
        return ("bad",)
    xlen = struct.unpack_from("<H", data, at + 10)[0]
    if len(data) - at < 12 + xlen:
        return ("short",)
    x, total = 0, 0
    while x + 4 <= xlen:
        slen = struct.unpack_from("<H", data, at + 12 + x + 2)[0]
        if x + 4 + slen > xlen:
            return ("bad",)
        if data[at + 12 + x:at + 12 + x + 2] == b"BC" and slen == 2:
            total = struct.unpack_from("<H", data, at + 12 + x + 4)[0] + 1
            break
        x += 4 + slen
    if not total or total < 12 + xlen + 8:
        return ("bad",)
    if len(data) - at < total:
        return ("short",)
    return ("ok", total, 12 + xlen)


def scan(data: bytes):
    """moni_bgzf_scan: (ok, members, used, sum of ISIZE)"""
    at = n = ob = 0
    while at < len(data):
        m = member_at(data, at)
        if m[0] != "ok":
            return m[0] != "bad", n, at, ob
        ob += struct.unpack_from("<I", data, at + m[1] - 4)[0]
        at += m[1]
        n += 1
    return True, n, at, ob


def inflate(data: bytes, check_crc: bool = True):
    """moni_bgzf_inflate: {'text', 'blocks', 'bad_blocks', 'first_bad_block', 'bad_reason', 'stored', 'fixed', 'dynamic', 'types': per member}"""
    at, texts, types, bad = 0, [], [], []
    while at < len(data):
        m = member_at(data, at)
        if m[0] != "ok":
            bad.append((len(types), HEADER if m[0] == "bad" else TRUNCATED))
            types.append([])
            break
        total, po = m[1], m[2]
        crc, isize = struct.unpack_from("<II", data, at + total - 8)
        text, tt, reason = inflate_payload(data[at + po:at + total - 8], isize)
        if reason == OK and check_crc and (zlib.crc32(text) & 0xFFFFFFFF) != crc:
            reason = CRC
        if reason != OK:
            bad.append((len(types), reason))
        texts.append(text)
        types.append(tt)
        at += total
    flat = [t for tt in types for t in tt]
    return {"text": b"".join(texts) if not bad else b"", "blocks": len(types), "bad_blocks": len(bad), "first_bad_block": bad[0][0] if bad else 0,
            "bad_reason": bad[0][1] if bad else OK, "stored": flat.count(0), "fixed": flat.count(1), "dynamic": flat.count(2), "types": types}


# ---- writing ------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v: int, n: int):
        """n bits of v, least significant first"""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n

    def put_code(self, code: int, n: int):
        """a Huffman code of n bits, most significant first"""
        for i in range(n - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self):
        self.n = (self.n + 7) & ~7

    def bytes(self) -> bytes:
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def codes_of(lengths):
    """canonical codes (RFC 1951 3.2.2) of a set of lengths; no check that the set is a code"""
    cnt = [0] * 17
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 17):
        c = (c + cnt[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lengths:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


def len_symbol(n: int):
    k = max(i for i in range(29) if LEN_BASE[i] <= n and (i == 28 or n < 258))
    return 257 + k, n - LEN_BASE[k], LEN_EXTRA[k]


def dist_symbol(d: int):
    k = max(i for i in range(30) if DIST_BASE[i] <= d)
    return k, d - DIST_BASE[k], DIST_EXTRA[k]


def put_tokens(W: BitWriter, tokens, ll, dl):
    """tokens: an int (literal), (length, distance), or ('sym', literal/length symbol) / ('dsym', length, distance symbol) to force a symbol;
    then the end-of-block code"""
    lc, dc = codes_of(ll), codes_of(dl)
    for t in tokens:
        if isinstance(t, int):
            W.put_code(lc[t], ll[t])
        elif t[0] == "sym":
            W.put_code(lc[t[1]], ll[t[1]])
        else:
            n = t[1] if t[0] == "dsym" else t[0]
            s, ev, eb = len_symbol(n)
            W.put_code(lc[s], ll[s])
            W.put(ev, eb)
            if t[0] == "dsym":
                W.put_code(dc[t[2]], dl[t[2]])
            else:
                s, ev, eb = dist_symbol(t[1])
                assert dl[s], "no code for distance symbol %d" % s
                W.put_code(dc[s], dl[s])
                W.put(ev, eb)
    W.put_code(lc[256], ll[256])


def fixed_block(tokens, last: bool = True, W: BitWriter = None) -> BitWriter:
    W = W or BitWriter()
    W.put(1 if last else 0, 1)
    W.put(1, 2)
    put_tokens(W, tokens, FIXED_LIT, FIXED_DIST)
    return W


def dynamic_block(tokens, ll, dl, last: bool = True, W: BitWriter = None, cl_syms=None, cl=None, nlit=None, ndist=None) -> BitWriter:
    """A dynamic block with the literal/length lengths ll and the distance lengths dl (at least one entry).  cl_syms: the code-length symbols
    to send, as ints 0..15 or (16 | 17 | 18, repeat count); by default one symbol per length.  cl: the lengths of the code-length code; by
    default 4 bits for the symbols 0..12 and 5 bits for 13..18 (13 / 16 + 6 / 32 = 1)."""
    W = W or BitWriter()
    nlit = len(ll) if nlit is None else nlit
    ndist = len(dl) if ndist is None else ndist
    assert 257 <= nlit <= 288 and 1 <= ndist <= 32
    if cl is None:
        cl = [4] * 13 + [5] * 6          # 13 / 16 + 6 / 32 = 1
    cc = codes_of(cl)
    if cl_syms is None:
        cl_syms = list(ll[:nlit]) + list(dl[:ndist])
    ncl = max(i + 1 for i in range(19) if cl[CL_ORDER[i]] or i < 4)
    W.put(1 if last else 0, 1)
    W.put(2, 2)
    W.put(nlit - 257, 5)
    W.put(ndist - 1, 5)
    W.put(ncl - 4, 4)
    for i in range(ncl):
        W.put(cl[CL_ORDER[i]], 3)
    for s in cl_syms:
        if isinstance(s, int):
            W.put_code(cc[s], cl[s])
        else:
            W.put_code(cc[s[0]], cl[s[0]])
            W.put(s[1] - (11 if s[0] == 18 else 3), {16: 2, 17: 3, 18: 7}[s[0]])
    ll = list(ll) + [0] * (288 - len(ll))
    dl = list(dl) + [0] * (32 - len(dl))
    put_tokens(W, tokens, ll, dl)
    return W


def stored_block(data: bytes, last: bool = True, W: BitWriter = None, nlen=None) -> BitWriter:
    W = W or BitWriter()
    W.put(1 if last else 0, 1)
    W.put(0, 2)
    W.align()
    W.put(len(data), 16)
    W.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    for b in data:
        W.put(b, 8)
    return W


def frame(payload: bytes, data: bytes, extra: bytes = b"") -> bytes:
    """bgzf_model.frame with other subfields before `BC`"""
    if not extra:
        return bm.frame(payload, data)
    xlen = len(extra) + 6
    total = 12 + xlen + len(payload) + 8
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra + b"BC\x02\0" + struct.pack("<H", total - 1) + payload +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def deflate_raw(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def bgzip(data: bytes, block_size: int = 65280, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY, eof: bool = False) -> bytes:
    out = [bm.frame(deflate_raw(data[at:at + block_size], level, strategy), data[at:at + block_size]) for at in range(0, len(data), block_size)]
    return b"".join(out) + (bm.EOF_BLOCK if eof else b"")
