"""Compressed streams written from explicit token lists, for the decoder tests (test_foreign_streams.py, test_gpu_foreign_streams.py).

The encoders of this project and of the checker write only a small part of what the three formats allow. The writers here follow the
formats as a decoder reads them instead: a stream is whatever token list a test asks for, including forms no encoder picks (non-greedy
LZNT1 parses, over-long Xpress length encodings, 32-bit lengths that wrap, incomplete Huffman codes, chunks that start off the 64 KiB
grid, ...). Every writer returns (stream, plaintext); the seeded family generators return lists of Stream records.

Tokens: ``("lit", byte)`` or ``("match", offset, length)``, with an optional encoding choice as a further element (see each writer).
"""
import random
import struct
from collections import Counter, namedtuple

# one stream of a family: the bytes, the capacity it is decoded with, the plaintext it means when valid (None: not meant to decode), and
# the features it holds (counted by test_foreign_streams.py)
Stream = namedtuple("Stream", "data cap plain tags")
# what the writers actually wrote, counted as they write it (the families' features, read by test_foreign_streams.py)
STATS = Counter()


# ===================================================================================================================================
# LZNT1: 2-byte chunk headers (size - 3 in bits 0-11, 0x3000 signature, bit 15 = compressed), each compressed chunk a series of flag
# bytes that each announce up to 8 tokens (bit set = a 16-bit match whose offset / length split depends on the position in the chunk)
# ===================================================================================================================================
def lznt1_split(pos):
    """(shift, largest offset, largest length) of a match token written at position pos of a chunk"""
    pow2, s = 0x10, 12
    while pow2 < pos:
        pow2 <<= 1
        s -= 1
    return s, 1 << (16 - s), (1 << s) + 2


def lznt1_chunk_payload(tokens, rnd=None):
    """the payload of one compressed chunk and its plaintext; the flag bits of a last, partly used flag byte are random when rnd is given
    (a decoder stops at the end of the payload before it looks at them)"""
    out, plain, i = bytearray(), bytearray(), 0
    while i < len(tokens):
        group = tokens[i:i + 8]
        i += 8
        flags, body = 0, bytearray()
        for k, t in enumerate(group):
            if t[0] == "lit":
                body.append(t[1])
                plain.append(t[1])
            else:
                _, off, ln = t[:3]
                pos = len(plain)
                s, max_off, max_len = lznt1_split(pos)
                assert 1 <= off <= min(pos, max_off) and 3 <= ln <= max_len and pos + ln <= 4096, (pos, off, ln)
                flags |= 1 << k
                body += struct.pack("<H", ((off - 1) << s) | (ln - 3))
                STATS["lznt1 offset to the chunk start"] += off == pos
                STATS["lznt1 largest length at a split"] += ln == max_len and pos in (16, 17) + tuple(1 << b for b in range(5, 12)) + tuple((1 << b) + 1 for b in range(5, 12))
                for _ in range(ln):
                    plain.append(plain[-off])
        if rnd is not None and len(group) < 8:
            flags |= rnd.getrandbits(8) & ~((1 << len(group)) - 1) & 0xFF
        out.append(flags)
        out += body
        STATS["lznt1 full chunk with flag bits left"] += len(plain) == 4096 and len(group) < 8 and i >= len(tokens)
    STATS["lznt1 payload of 4096 bytes"] += len(out) == 4096
    STATS["lznt1 payload longer than its output"] += len(out) > len(plain)
    return bytes(out), bytes(plain)


def lznt1_header(payload_len, compressed):
    assert 1 <= payload_len <= 4096
    return struct.pack("<H", (payload_len - 1) | 0x3000 | (0x8000 if compressed else 0))


def lznt1_write(chunks, end="00", rnd=None):
    """chunks: list of ("c", tokens) (compressed) or ("s", raw bytes) (stored, any length 1..4096). end: "00" = the 00 00 terminator,
    "0" = a single 0 byte, "" = none. Returns (stream, plaintext)."""
    out, plain = bytearray(), bytearray()
    for ci, (kind, body) in enumerate(chunks):
        mid = ci < len(chunks) - 1
        if kind == "c":
            pay, p = lznt1_chunk_payload(body, rnd)
            out += lznt1_header(len(pay), True) + pay
            plain += p
            STATS["lznt1 short compressed chunk in the middle"] += mid and len(p) < 4096
        else:
            out += lznt1_header(len(body), False) + body
            plain += body
            STATS["lznt1 stored chunk in the middle"] += mid
    out += {"00": b"\0\0", "0": b"\0", "": b""}[end]
    STATS["lznt1 end '%s'" % end] += 1
    return bytes(out), bytes(plain)


def _lznt1_random_tokens(rnd, n_out, lit_p=0.4, max_len=None):
    """a non-greedy parse of about n_out bytes: literals and matches of random legal offset and length at their position"""
    toks, pos = [], 0
    while pos < n_out:
        if pos == 0 or rnd.random() < lit_p:
            toks.append(("lit", rnd.choice(b"abcdxyz\0\xff")))
            pos += 1
            continue
        _, mo, ml = lznt1_split(pos)
        ml = min(ml, 4096 - pos, max_len or ml)
        if ml < 3:
            toks.append(("lit", rnd.getrandbits(8)))
            pos += 1
            continue
        ln = rnd.randint(3, ml) if rnd.random() < 0.3 else rnd.randint(3, min(ml, 20))
        toks.append(("match", rnd.randint(1, min(pos, mo)), ln))
        pos += ln
    return toks


def lznt1_family(seed=1):
    """valid LZNT1 streams of every listed feature, each at its exact capacity, with invalid variants around some of them"""
    rnd = random.Random(seed)
    valid = []

    def add(chunks, tags, end="00"):
        s, p = lznt1_write(chunks, end, rnd)
        # (a 00 00 terminator is only read while there is room left: at a capacity of exactly the plaintext the call ends in BUF_ERROR)
        valid.append((s, p, frozenset(tags), len(p) + (end == "00")))

    # non-greedy parses, one to several chunks, short chunks inside
    for k in range(24):
        chunks = []
        for c in range(rnd.randint(1, 4)):
            n = 4096 if rnd.random() < 0.5 else rnd.randint(1, 4096)
            chunks.append(("c", _lznt1_random_tokens(rnd, n)))
        add(chunks, {"nongreedy"} | ({"short_chunk_mid"} if any(len(lznt1_chunk_payload(t)[1]) < 4096 for _, t in chunks[:-1]) else set()),
            end=("00", "0", "")[k % 3])
    # the largest length at every displacement split (positions 16/17 ... 2048/2049), and an offset reaching exactly to the chunk start
    for p in [16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049]:
        toks = [("lit", rnd.getrandbits(8)) for _ in range(p)]
        _, mo, ml = lznt1_split(p)
        toks.append(("match", min(mo, p), min(ml, 4096 - p)))
        rest = 4096 - p - min(ml, 4096 - p)
        toks += [("lit", rnd.getrandbits(8)) for _ in range(min(rest, 40))]
        add([("c", toks)], {"max_len_split", "off_to_start"} if min(mo, p) == p else {"max_len_split"})
    for p in (1, 5, 16, 300, 3000):
        toks = [("lit", rnd.getrandbits(8)) for _ in range(p)] + [("match", p, 3)]
        add([("c", toks), ("c", [("lit", 1), ("match", 1, 50)])], {"off_to_start"})
    # compressed chunks whose payload is the full 4096 bytes (3639 literals + one match: 3639 + 455 flag bytes + 2), longer than their output
    for k in range(3):
        toks = [("lit", rnd.getrandbits(8)) for _ in range(3639)]
        toks.insert(rnd.randint(1, 3638), ("match", 1, 3 + k))
        add([("c", toks), ("c", _lznt1_random_tokens(rnd, 2000))][: 1 + k % 2], {"payload_4096", "payload_gt_out"})
    for k in range(3):                                                   # ... and shorter payloads that are still longer than the output
        n = rnd.randint(200, 3000)
        add([("c", [("lit", rnd.getrandbits(8)) for _ in range(n)]), ("c", _lznt1_random_tokens(rnd, 4096))], {"payload_gt_out"})
    # stored chunks and short compressed chunks in the middle
    for k in range(6):
        chunks = [("c", _lznt1_random_tokens(rnd, rnd.randint(1, 4095))),
                  ("s", bytes(rnd.getrandbits(8) for _ in range(rnd.choice([1, 17, 4095, 4096])))),
                  ("c", _lznt1_random_tokens(rnd, 4096))]
        add(chunks, {"stored_mid", "short_chunk_mid"})
    # a chunk full at 4096 bytes with flag bits left over (the last match ends at 4096 inside a flag byte; the rest of its bits random)
    for k in range(6):
        while True:
            toks = _lznt1_random_tokens(rnd, 4096)
            if len(toks) % 8 and sum(1 if t[0] == "lit" else t[2] for t in toks) == 4096:
                break
        add([("c", toks), ("c", _lznt1_random_tokens(rnd, 100))][: 1 + k % 2], {"full_flags_left"})
    # the three stream ends
    for end in ("00", "0", ""):
        add([("c", _lznt1_random_tokens(rnd, 700))], {"end_" + end})
    # a stream that goes over several input segments (the speculative header chain works per 48 KiB of input): 160 chunks
    chunks = [("c", _lznt1_random_tokens(rnd, 4096, lit_p=0.7)) if c % 5 else ("s", bytes(rnd.getrandbits(8) for _ in range(4096)))
              for c in range(160)]
    add(chunks, {"multi_segment", "stored_mid"})
    return _with_variants(2, valid, rnd)


# ===================================================================================================================================
# Xpress (plain LZ77): 32-bit flag words (bit 31 first, set = match), 16-bit match symbols (offset - 1 << 3 | length - 3, 7 = more),
# shared length nibbles, then a byte, a 16-bit and a 32-bit length form
# ===================================================================================================================================
def xpress_write(tokens, tail=None):
    """tokens: ("lit", b) or ("match", off, len[, form]) with form None (canonical), "byte", "16" or "32" for the form of the extended
    length; a match may also be ("raw32", off, L) whose 32-bit length field holds L as it stands (what the reference makes of it: len =
    L + 3 mod 2^32). tail: the flag bits after the last token, as a list of 0/1 (default: all ones, the only legal pattern). The nibble
    byte that a last token leaves half used gets a random high half. Returns (stream, plaintext); the plaintext is None when a token's
    length wraps beyond what the writer plays back (its caller knows the answer)."""
    out = bytearray()
    plain = bytearray()
    half = None                                                          # position of a nibble byte whose high half is still free
    flag_pos, nflag, flags = None, 32, 0
    rnd = random.Random(len(tokens))
    toks = list(tokens)
    i = 0
    while True:
        if nflag == 32:
            if flag_pos is not None:
                struct.pack_into("<I", out, flag_pos, flags)
            flag_pos, nflag, flags = len(out), 0, 0
            out += b"\0\0\0\0"
        if i == len(toks):
            break
        t = toks[i]
        i += 1
        if t[0] == "lit":
            out.append(t[1])
            if plain is not None:
                plain.append(t[1])
        else:
            flags |= 1 << (31 - nflag)
            kind, off, ln = t[:3]
            form = t[3] if len(t) > 3 else None
            L = ln if kind == "raw32" else ln - 3
            assert 1 <= off <= 8192 and (kind == "raw32" or (0 <= L and (form is None or L >= 22)))
            STATS["xpress 16-bit length below 280"] += form == "16" and L + 3 < 280
            STATS["xpress 32-bit length below 65536"] += form == "32" and L + 3 < 65536
            STATS["xpress 32-bit length that wraps"] += kind == "raw32" and L >= 0xFFFFFFFD
            if off in (1, 2, 3, 8192):
                STATS["xpress offset %d" % off] += 1
            STATS["xpress overlapping match"] += off < ((L + 3) & 0xFFFFFFFF)
            out += struct.pack("<H", ((off - 1) << 3) | min(L, 7))
            if L >= 7 or kind == "raw32":
                n = min(L - 7, 15) if kind != "raw32" else 15
                if half is None:
                    half = len(out)
                    out.append(n)
                else:
                    out[half] |= n << 4
                    half = None
                if n == 15:
                    if kind == "raw32" or form in ("16", "32") or L - 22 >= 255:
                        out.append(255)
                        if kind == "raw32" or form == "32" or L > 0xFFFF:
                            out += struct.pack("<HI", 0, L & 0xFFFFFFFF)
                        else:
                            out += struct.pack("<H", L)
                    else:
                        out.append(L - 22)
            total = (L + 3) & 0xFFFFFFFF
            if plain is not None and total <= 1 << 24:
                if off > len(plain):
                    plain = None
                else:
                    for _ in range(total):
                        plain.append(plain[-off])
            else:
                plain = None
        nflag += 1
    tail = [1] * (32 - nflag) if tail is None else list(tail)
    assert len(tail) == 32 - nflag
    for k, b in enumerate(tail):
        flags |= b << (31 - nflag - k)
    struct.pack_into("<I", out, flag_pos, flags)
    if half is not None:
        out[half] |= rnd.randint(1, 15) << 4                             # the unused high half of a shared length nibble
        STATS["xpress length nibble never used"] += 1
    return bytes(out), (bytes(plain) if plain is not None else None)


def _xp_len_forms(L):
    """every length form that can hold L = length - 3"""
    if L < 7:
        return [None]
    if L < 22:
        return [None]
    forms = [None, "32"] + (["16"] if L <= 0xFFFF else [])
    return forms


def _xpress_random_tokens(rnd, n_out, lit_p=0.4, long_p=0.05, max_off=8192):
    toks, pos = [], 0
    while pos < n_out:
        if pos == 0 or rnd.random() < lit_p:
            toks.append(("lit", rnd.choice(b"abcdxyz\0\xff")))
            pos += 1
            continue
        off = rnd.choice([1, 2, 3, 8192, rnd.randint(1, 64), rnd.randint(1, max_off)])
        off = min(off, pos)
        r = rnd.random()
        ln = rnd.randint(270, 70000) if rnd.random() < long_p else rnd.randint(3, 9) if r < 0.5 else rnd.randint(10, 24) if r < 0.8 else rnd.randint(25, 400)
        form = rnd.choice(_xp_len_forms(ln - 3))
        toks.append(("match", off, ln, form))
        pos += ln
    return toks


def _xpress_large_tokens(rnd, n_in):
    """tokens of a stream of about n_in input bytes: runs of literals between matches of every form, a few long ones"""
    toks, pos, size = [("lit", 1)], 1, 0
    while size < n_in:
        k = rnd.randint(1, 120)
        toks += [("lit", b) for b in rnd.randbytes(k)]
        pos += k
        off = min(rnd.choice([1, 2, 3, 8192, rnd.randint(1, 8192)]), pos)
        ln = rnd.randint(3, 60) if rnd.random() < 0.97 else rnd.randint(200, 5000)
        toks.append(("match", off, ln, rnd.choice(_xp_len_forms(ln - 3))))
        pos += ln
        size += k * 33 // 32 + 4
    return toks


def xpress_family(seed=2):
    rnd = random.Random(seed)
    valid = []

    def add(tokens, tags, tail=None):
        s, p = xpress_write(tokens, tail)
        assert p is not None
        valid.append((s, p, frozenset(tags)))

    lead = [("lit", c) for c in b"0123456789abcdefghij"]
    # every length form, canonical and not, at the lengths around each boundary
    for L in [0, 6, 7, 8, 21, 22, 23, 100, 276, 277, 278, 279, 280, 1000, 65535, 65536, 65537, 100000]:
        for form in _xp_len_forms(L):
            toks = lead + [("match", rnd.choice([1, 2, 3, 20]), L + 3, form)] + [("lit", 65)]
            tags = {"len_form_" + str(form)}
            if form == "16" and L + 3 < 280:
                tags.add("len16_short")
            if form == "32" and L < 65536:
                tags.add("len32_short")
            add(toks, tags)
    # 32-bit lengths 0xFFFFFFFD .. 0xFFFFFFFF wrap to matches of 0 .. 2 bytes (the reference keeps the length in 32 bits)
    for L in (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF):
        for off in (1, 7, 20):
            s, _ = xpress_write(lead + [("raw32", off, L), ("lit", 66), ("match", 1, 5)])
            p = bytearray(bytes(range(48, 58)) + b"abcdefghij")
            for _ in range((L + 3) & 0xFFFFFFFF):
                p.append(p[-off])
            p.append(66)
            p += bytes([p[-1]]) * 5
            valid.append((s, bytes(p), frozenset({"len32_wrap"})))
    nowrap = [Stream(xpress_write(lead + [("raw32", 1, 0xFFFFFFFC), ("lit", 66)])[0], cap, None, frozenset({"len32_nowrap"}))
              for cap in (100, 1 << 20)]
    # offsets 1, 2, 3 and 8192, overlapping matches
    body = [("lit", rnd.getrandbits(8)) for _ in range(8200)]
    for off in (1, 2, 3, 8192):
        add(body + [("match", off, rnd.choice([3, 10, 30, 9000]))] + [("match", off, 2 * off + 5)], {"off_%d" % off, "overlap"})
    # a pending nibble never used (odd number of nibble matches)
    for k in range(4):
        toks = lead + [("match", 5, 10 + k)] + [("lit", 1)] * k
        add(toks, {"half_unused"})
    # random non-greedy token streams of all forms
    for k in range(30):
        add(_xpress_random_tokens(rnd, rnd.choice([10, 100, 1000, 5000, 40000])), {"nongreedy"})
    # the end of the stream: k tokens in the last flag word, the flag bits after them all set (legal) or with a clear bit (illegal)
    ends = []
    for k in (0, 1, 2, 5, 30, 31):
        toks = [("lit", rnd.getrandbits(8)) for _ in range(32 + k)]
        s, p = xpress_write(toks)
        valid.append((s, p, frozenset({"end_flags_legal"})))
        for z in sorted({0, 31 - k, rnd.randint(0, 31 - k)}):
            tail = [1] * (32 - k)
            tail[z] = 0
            ends.append(Stream(xpress_write(toks, tail)[0], len(p) + 10, None, frozenset({"end_flags_illegal"})))
        if k < 31:
            tail = [1] * (32 - k)
            tail[-1] = 0                                                 # the lowest bit: the sentinel would not be reached
            ends.append(Stream(xpress_write(toks, tail)[0], len(p) + 10, None, frozenset({"end_flags_illegal"})))
    ends.append(Stream(xpress_write([("lit", 1)] * 32)[0][:-4], 100, None, frozenset({"end_flags_illegal"})))   # a full word, no end word
    # streams shorter than the minimum and the 4-byte streams
    short = [Stream(b"", 10, b"", frozenset({"short"}))]
    for n in (1, 2, 3):
        short.append(Stream(bytes(rnd.getrandbits(8) for _ in range(n)), 10, None, frozenset({"short"})))
    for w in (0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFE, 0, 0x80000000):
        short.append(Stream(struct.pack("<I", w), 10, b"" if w != 0xFFFFFFFF else None, frozenset({"four_byte"})))
    add([("lit", 9)], {"five_byte"})
    # one stream of 512 KiB input or more (the segment walk of large streams), mostly literals and nibble-sized matches, a few long ones
    add(_xpress_large_tokens(random.Random(seed + 1), 600_000), {"large_input"})
    return _with_variants(3, valid, rnd) + ends + short + nowrap


# ===================================================================================================================================
# Xpress+Huffman: per chunk 256 bytes of code lengths (512 nibbles) and a bit stream read in 16-bit little-endian words into a 32-bit
# mask; extended lengths are raw bytes taken from the input position as it stands when the length is decoded (the reader's fetch
# schedule is simulated below, so that every word lands where the reader fetches it)
# ===================================================================================================================================
def canonical_codes(lens):
    """code of every symbol of a (possibly incomplete) code: shorter codes first, then by symbol, counting up from 0"""
    codes, code = {}, 0
    order = sorted((l, s) for s, l in enumerate(lens) if l)
    prev = 0
    for l, s in order:
        code <<= (l - prev)
        prev = l
        codes[s] = (code, l)
        code += 1
    return codes


def kraft(lens):
    return sum(1 << (15 - l) for l in lens if l)


class _XhWriter:
    """writes bits and raw bytes where the reader takes them (Bitstream.h's InputBitstream: two words at the start of a chunk, one more
    whenever fewer than 16 bits are left)"""

    def __init__(self, out):
        self.out = out
        self.words = []                                                  # positions of the words the reader has fetched, in order
        self.bitpos = 0                                                  # bits consumed since the chunk's bit stream started
        self.start_chunk()

    def start_chunk(self):
        self.base_bit = self.bitpos
        self.words = [len(self.out), len(self.out) + 2]
        self.out += b"\0\0\0\0"
        self.bits = 32

    def put(self, v, k):
        """k bits (the reader has them in its mask: k <= bits)"""
        assert k <= self.bits, (k, self.bits)
        for j in range(k):
            if (v >> (k - 1 - j)) & 1:
                b = self.bitpos - self.base_bit + j
                w = self.words[b // 16]
                bit = 15 - b % 16
                self.out[w + bit // 8] |= 1 << (bit % 8)
        self.bitpos += k
        self.bits -= k
        if self.bits < 16:                                               # (the stream goes on beyond: the writer ends where the reader is)
            self.words.append(len(self.out))
            self.out += b"\0\0"
            self.bits += 16

    def raw(self, b):
        self.out += b

    def window(self):
        """the bits the reader holds but has not consumed (judged once the chunk is written: later tokens fill them)"""
        return self.bitpos - self.base_bit, self.bits

    def pending_nonzero(self, win=None):
        """are there set bits among them?"""
        lo, n = win or self.window()
        for b in range(lo, lo + n):
            w = self.words[b // 16]
            bit = 15 - b % 16
            if self.out[w + bit // 8] >> (bit % 8) & 1:
                return True
        return False


def xh_symbol(off, ln):
    L = (ln - 3) & 0xFFFFFFFF
    ob = off.bit_length() - 1
    return 0x100 | (ob << 4) | min(L, 15)


def xpress_huff_write(chunks):
    """chunks: list of (lens, tokens): lens = 512 code lengths (0..15; complete or not), tokens ("lit", b), ("match", off, len[, form])
    with form None / "16" / "32" (the extended-length form; needs len - 3 >= 15 ... and for "16" len - 3 <= 0xFFFF), or ("raw32", off, L)
    (32-bit length field L: len = L + 3 mod 2^32). A chunk ends after its tokens: all but the last must have produced at least 65536
    bytes by then, and the last ends with the end-of-stream symbol 0x100. A token of a chunk that has already produced 65536 bytes is only
    read when the reader's pending bits are non-zero: the writer checks that. Returns (stream, plaintext)."""
    out, plain = bytearray(), bytearray()
    w = None
    for ci, (lens, tokens) in enumerate(chunks):
        assert len(lens) == 512 and kraft(lens) <= 32768
        codes = canonical_codes(lens)
        STATS["xpress_huff incomplete code"] += kraft(lens) < 32768
        STATS["xpress_huff 15-bit code length"] += max(lens) == 15
        STATS["xpress_huff one-symbol code"] += len(codes) == 1
        STATS["xpress_huff code without 0x100"] += lens[0x100] == 0
        STATS["xpress_huff chunk that starts off the grid"] += len(plain) % 65536 != 0
        out += bytes(lens[2 * i] | (lens[2 * i + 1] << 4) for i in range(256))
        if w is None:
            w = _XhWriter(out)
        else:
            w.start_chunk()
        start = len(plain)
        checks = []
        for t in tokens:
            if len(plain) - start >= 65536:
                checks.append(w.window())
                STATS["xpress_huff token read past the mark"] += 1
            if t[0] == "lit":
                w.put(*codes[t[1]])
                plain.append(t[1])
                continue
            kind, off, ln = t[:3]
            form = t[3] if len(t) > 3 else None
            L = (ln if kind == "raw32" else ln - 3) & 0xFFFFFFFF
            ob = off.bit_length() - 1
            w.put(*codes[0x100 | (ob << 4) | min(L, 15)])
            STATS["xpress_huff 0x100 as a match"] += (0x100 | (ob << 4) | min(L, 15)) == 0x100
            STATS["xpress_huff offset bits %d" % ob] += 1
            STATS["xpress_huff offset 65535"] += off == 65535
            STATS["xpress_huff 16-bit length below 270"] += form == "16" and L < 270
            STATS["xpress_huff 32-bit length below 65536"] += form == "32" and L < 65536
            STATS["xpress_huff 32-bit length that wraps"] += kind == "raw32" and L >= 0xFFFFFFFD
            if L >= 15:
                if kind == "raw32" or form in ("16", "32") or L - 15 >= 255:
                    w.raw(b"\xff")
                    if kind == "raw32" or form == "32" or L > 0xFFFF:
                        w.raw(struct.pack("<HI", 0, L))
                    else:
                        w.raw(struct.pack("<H", L))
                else:
                    w.raw(bytes([L - 15]))
            w.put(off - (1 << ob), ob)
            assert off <= len(plain), (off, len(plain))
            if (L + 3) & 0xFFFFFFFF > 1 << 24:                           # (a length that does not wrap: no capacity holds it)
                plain = None
                break
            for _ in range((L + 3) & 0xFFFFFFFF):
                plain.append(plain[-off])
        if plain is None:
            return bytes(out), None
        assert all(w.pending_nonzero(c) for c in checks), "the reader would end the chunk before all its tokens"
        if ci == len(chunks) - 1:
            w.put(*codes[0x100])
        else:
            assert len(plain) - start >= 65536 and not w.pending_nonzero()
            # the next chunk's table starts where the reader's input pointer is; what it still holds in its mask is dropped
    return bytes(out), bytes(plain)


def _random_lengths(rnd, symbols, complete=True, max_len=15):
    """code lengths for the given symbols (at least one): a random complete code (or an incomplete one: some code space left over)"""
    syms = list(symbols)
    rnd.shuffle(syms)
    lens = [0] * 512
    if len(syms) == 1:
        lens[syms[0]] = rnd.randint(1, max_len) if not complete else 1
        return lens
    # split the code space at random: a random binary tree with the symbols at the leaves, depth <= max_len
    leaves = [0]
    while len(leaves) < len(syms):
        cand = [i for i, d in enumerate(leaves) if d < max_len]
        i = rnd.choice(cand) if rnd.random() < 0.5 else min(cand, key=lambda j: leaves[j])
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    for s, d in zip(syms, leaves):
        lens[s] = max(d, 1)
    if not complete:                                                    # drop the code space of one leaf: make it one longer than needed
        s = max(syms, key=lambda x: -lens[x])
        if lens[s] < 15:
            lens[s] += 1
        else:
            lens[syms[0]] = 0 if len(syms) > 2 else lens[syms[0]]
    return lens


def _xh_chunk_symbols(tokens, extra=()):
    syms = set(extra) | {0x100}
    for t in tokens:
        if t[0] == "lit":
            syms.add(t[1])
        else:
            L = (t[2] if t[0] == "raw32" else t[2] - 3) & 0xFFFFFFFF
            syms.add(0x100 | ((t[1].bit_length() - 1) << 4) | min(L, 15))
    return syms


def _xh_random_tokens(rnd, n_out, have, lit_p=0.4, long_p=0.05):
    """tokens that produce at least n_out bytes after `have` bytes of earlier output; the last one may overshoot by up to its length"""
    toks, pos = [], have
    end = have + n_out
    while pos < end:
        if pos == 0 or rnd.random() < lit_p:
            toks.append(("lit", rnd.getrandbits(8)))
            pos += 1
            continue
        ob = rnd.randint(0, 15)
        off = min(rnd.randint(1 << ob, (1 << (ob + 1)) - 1), pos)
        r = rnd.random()
        ln = rnd.randint(300, 70000) if rnd.random() < long_p else rnd.randint(3, 17) if r < 0.6 else rnd.randint(18, 300)
        form = rnd.choice([None, None, "16", "32"]) if ln - 3 >= 15 and ln - 3 <= 0xFFFF else None
        toks.append(("match", off, ln, form))
        pos += ln
    return toks, pos - have


def xh_chunks_from_tokens(rnd, token_chunks, complete=True, extra=(), max_len=15):
    out = []
    for toks in token_chunks:
        syms = _xh_chunk_symbols(toks, extra)
        lens = _random_lengths(rnd, syms, complete if not callable(complete) else complete(), max_len)
        out.append((lens, toks))
    return out


def xh_multichunk(rnd, n_chunks, complete=True, off_grid=True, literals=600, last_past=True):
    """a buffer of n_chunks chunks that produce 65536 bytes each plus, when off_grid, an overshoot by the last match of every chunk (so that
    every chunk after the first starts off the 64 KiB grid); few tokens: long matches make up most of every chunk. last_past: the last
    chunk, too, reaches the mark (it then reads its end-of-stream symbol with bits pending); else it ends a few KiB short of it"""
    token_chunks, have = [], 0
    for c in range(n_chunks):
        toks = [("lit", rnd.getrandbits(8)) for _ in range(max(1, literals) if c == 0 else rnd.randint(0, literals))]
        pos = have + len(toks)
        target = have + 65536
        while pos < target - 4100:
            off = rnd.choice([1, 2, 3, rnd.randint(1, 70), rnd.randint(1, min(pos, 65535)), min(pos, 65535)])
            off = min(off, pos, 65535)
            ln = rnd.randint(3, 4000) if rnd.random() < 0.8 else rnd.randint(20, 600)
            toks.append(("match", off, ln, rnd.choice([None, "16", "32"]) if 18 <= ln <= 0xFFFF + 3 else None))
            pos += ln
            if rnd.random() < 0.3:
                toks.append(("lit", rnd.getrandbits(8)))
                pos += 1
        # the last match crosses the mark: ends 1 .. 4000 bytes past it (off grid), or the chunk is filled exactly
        rest = target - pos
        if c == n_chunks - 1 and not last_past:
            pass
        elif c < n_chunks - 1 or off_grid:
            toks.append(("match", rnd.randint(1, min(pos, 65535)), rest + (rnd.randint(1, 4000) if off_grid else 0)))
        else:
            toks.append(("match", 1, rest))
        pos = sum(1 if t[0] == "lit" else t[2] for t in toks) + have
        token_chunks.append(toks)
        have = pos
    return xh_chunks_from_tokens(rnd, token_chunks, complete)


def xpress_huff_family(seed=3, big=True):
    """valid Xpress+Huffman streams of every listed feature (and invalid variants); big: also the multi-MB buffers"""
    rnd = random.Random(seed)
    valid = []

    def add(chunks, tags):
        s, p = xpress_huff_write(chunks)
        valid.append((s, p, frozenset(tags)))

    # single chunks: random complete codes, incomplete codes, codes with 15-bit lengths
    for k in range(16):
        toks, _ = _xh_random_tokens(rnd, rnd.choice([1, 10, 500, 5000, 40000]), 0)
        complete = k % 2 == 0
        max_len = 15
        chunks = xh_chunks_from_tokens(rnd, [toks], complete, max_len=max_len)
        lens = chunks[0][0]
        tags = {"complete" if kraft(lens) == 32768 else "incomplete"}
        if max(lens) == 15:
            tags.add("len15")
        add(chunks, tags)
    # a code with 15-bit lengths for sure: a deep chain of a tree
    lens = [0] * 512
    for d in range(14):
        lens[d] = d + 1
    lens[0x100] = lens[0x103] = 15                                       # 1 .. 14, 15, 15: complete
    toks = [("lit", s) for s in range(14)] * 5 + [("match", 1, 6)] * 3
    add([(lens, toks)], {"len15", "complete"})
    # one-symbol codes: the end-of-stream symbol alone; a literal alone in a full chunk; a long match alone in a full chunk
    add([([1 if s == 0x100 else 0 for s in range(512)], [])], {"one_symbol"})
    t0 = [("lit", 7)] * 10
    c0 = xh_chunks_from_tokens(rnd, [t0 + [("match", 1, 65536 - 10)]])
    one_lit = ([1 if s == 0x41 else 0 for s in range(512)], [("lit", 0x41)] * 65536)
    m = ("match", 1, 65536, "16")
    one_match = ([1 if s == xh_symbol(1, 65536) else 0 for s in range(512)], [m])
    last = xh_chunks_from_tokens(rnd, [[("lit", 3), ("match", 2, 40)]])
    add(c0 + [one_lit] + last, {"one_symbol", "complete"})
    add(c0 + [one_match] + last, {"one_symbol", "complete"})
    # codes without symbol 0x100 (in a chunk that is not the last), and 0x100 used as a match (length 3, offset 1) in the middle of a stream
    toks = [("lit", 5)] * 100 + [("match", 1, 65436 + 7)]
    lens = _random_lengths(rnd, {5, xh_symbol(1, 65436 + 7)}, True)
    mid = [("lit", 1), ("match", 1, 3), ("match", 1, 3), ("lit", 2), ("match", 1, 3), ("lit", 3)]
    add([(lens, toks)] + xh_chunks_from_tokens(rnd, [mid]), {"no_eos_symbol", "eos_as_match", "off_grid"})
    for k in range(3):
        toks, _ = _xh_random_tokens(rnd, 2000, 0)
        toks = toks + [("match", 1, 3)] * (k + 1) + [("lit", 9)]
        add(xh_chunks_from_tokens(rnd, [toks]), {"eos_as_match"})
    # every offset-bit count 0 .. 15, offset 65535 included
    base = [("lit", rnd.getrandbits(8)) for _ in range(300)] + [("match", 300, 65236)]
    toks = [("match", (1 << ob) + rnd.randint(0, (1 << ob) - 1), 5) for ob in range(16)] + [("match", 65535, 20), ("match", 32768, 4)]
    add(xh_chunks_from_tokens(rnd, [base, toks]), {"all_off_bits", "off_65535"})
    # every extended-length form (byte, 16-bit, 32-bit; canonical and not), 32-bit lengths that wrap
    lead = [("lit", c) for c in b"abcdefghijklmnopqrst"]
    for L in [14, 15, 16, 269, 270, 271, 1000, 65535, 65536, 100000]:
        for form in [None, "16", "32"]:
            if form == "16" and L > 0xFFFF:
                continue
            if form is not None and L < 15:
                continue
            tags = {"xlen_" + str(form)}
            if form == "16" and L < 270:
                tags.add("xlen16_short")
            if form == "32" and L <= 0xFFFF:
                tags.add("xlen32_short")
            tail = [("lit", 1)] if L + 23 < 65536 else []                 # (a token past the mark is read only if its code has a set bit)
            add(xh_chunks_from_tokens(rnd, [lead + [("match", rnd.choice([1, 3, 17]), L + 3, form)] + tail]), tags)
    for L in (0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF):
        add(xh_chunks_from_tokens(rnd, [lead + [("raw32", rnd.choice([1, 2, 20]), L), ("lit", 1), ("match", 1, 4)]]), {"xlen32_wrap"})
    nowrap = [Stream(xpress_huff_write(xh_chunks_from_tokens(rnd, [lead + [("raw32", 1, 0xFFFFFFFC), ("lit", 1)]]))[0], cap, None,
                     frozenset({"xlen32_nowrap"})) for cap in (100, 1 << 20)]
    # matches across the 64 KiB mark, chunks that go on while pre-read bits are non-zero; two and three chunks, complete and incomplete codes
    for k in range(6):
        add(xh_multichunk(rnd, 2 + k % 2, complete=k < 4, literals=rnd.choice([0, 50, 600])), {"off_grid"})
    add(xh_multichunk(rnd, 3, complete=True, off_grid=False), {"on_grid"})
    # a chunk that keeps decoding past 65536 bytes because its pending bits are not all zero: literals with codes that begin with a 1
    lens = [0] * 512
    lens[0x80], lens[0x81], lens[0x100], lens[0x101] = 1, 2, 3, 3         # 0x80 = 0, 0x81 = 10, 0x100 = 110, 0x101 = 111
    toks = [("lit", 0x81)] + [("lit", 0x80)] * 65535 + [("lit", 0x81)] * 40
    add([(lens, toks)] + xh_chunks_from_tokens(rnd, [[("match", 1, 10)]]), {"past_mark_pending", "off_grid"})
    families = _with_variants(4, valid, rnd) + nowrap
    if big:
        families += xpress_huff_big(seed + 100)
    return families


def xpress_huff_big(seed):
    """multi-MB buffers where every chunk after the first starts off the grid: all codes complete (the chunk-parallel path takes them), and
    one incomplete code among complete ones (the serial walk must take it). Their last chunk ends short of the mark: a chunk that is still
    reading past it is left to the serial walk on purpose (csrc/xhuff_decode.hip, xhc_parse_kernel)"""
    rnd = random.Random(seed)
    out = []
    for k, n in enumerate((40, 48)):
        s, p = xpress_huff_write(xh_multichunk(rnd, n, complete=True, literals=300, last_past=False))
        out.append(Stream(s, len(p), p, frozenset({"big", "big_complete", "off_grid"})))
    for k, n in enumerate((40, 44)):
        flags = [True] * n
        flags[rnd.randint(1, n - 1)] = False
        it = iter(flags)
        chunks = xh_multichunk(rnd, n, complete=lambda: next(it), literals=300, last_past=False)
        s, p = xpress_huff_write(chunks)
        out.append(Stream(s, len(p), p, frozenset({"big", "big_incomplete", "off_grid"})))
    return out


# ===================================================================================================================================
def _with_variants(fmt, valid, rnd):
    """every valid stream at the smallest capacity that decodes it (and some at more); around every third: one byte short, one byte too
    many, a capacity one short and (where that differs) a capacity of exactly the plaintext's length"""
    out = []
    for i, v in enumerate(valid):
        s, p, tags = v[:3]
        need = v[3] if len(v) > 3 else len(p)                           # the smallest capacity that decodes
        out.append(Stream(s, need, p, tags))
        if i % 3 == 0:
            out.append(Stream(s, need + rnd.choice([1, 100, 5000]), p, tags))
            out.append(Stream(s[:-1], need, None, frozenset({"variant_short"})))
            out.append(Stream(s + bytes([rnd.getrandbits(8)]), need, None, frozenset({"variant_long"})))
            if need:
                out.append(Stream(s, need - 1, None, frozenset({"variant_cap_short"})))
            if need != len(p):
                out.append(Stream(s, len(p), None, frozenset({"variant_cap_exact"})))
    return out


FAMILIES = {2: lznt1_family, 3: xpress_family, 4: xpress_huff_family}
