"""What the device's deflate encoder (include/video_io.h gsr_png_encode, csrc/gs_png.h) promises, restated on the host. Not a test itself:
tests/test_png_host.py and tests/test_hip_png.py use it.
  filtered    the scanlines png.encode passes to zlib: per row the filter type, then the row's bytes (16-bit samples big-endian)
  tokens      the token rule of one segment in numpy: byte q >= D repeats when b[q] == b[q - D]; a maximal run of repeating bytes is cut
              into pieces of 258 from its start; a piece of 3 or more is one match, everything else a literal
  parse       a small inflate that keeps the tokens: the blocks of a zlib stream as (type, tokens), independent of the encoder
  huffman_depth  the depth of the unconstrained Huffman tree of a histogram"""
import heapq
import zlib

import numpy as np

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def filtered(image, filter):
    """uint8 [H, row]: the filtered scanlines of a uint8 [H, W, 3] or uint16 [H, W] image, filter 0 (None) or 2 (Up)."""
    a = np.asarray(image)
    rows = a.reshape(a.shape[0], -1) if a.dtype == np.uint8 else a.astype(">u2").view(np.uint8).reshape(a.shape[0], -1)
    raw = np.empty((a.shape[0], rows.shape[1] + 1), np.uint8)
    raw[:, 0] = filter
    raw[:, 1:] = rows
    if filter == 2:
        raw[1:, 1:] = rows[1:] - rows[:-1]
    return raw


def tokens(segment, D):
    """The tokens of one segment's bytes, in order: ("lit", byte) or ("match", length); every match has distance D."""
    b = np.asarray(segment, np.uint8)
    rep = np.zeros(len(b), bool)
    rep[D:] = b[D:] == b[:-D]
    edges = np.flatnonzero(np.diff(np.concatenate(([0], rep.astype(np.int8), [0]))))
    literal = ~rep
    found = []
    for start, end in zip(edges[::2], edges[1::2]):                      # maximal runs [start, end)
        for p in range(start, end, 258):
            length = min(258, end - p)
            if length >= 3:
                found.append((int(p), "match", int(length)))
            else:
                literal[p:p + length] = True
    found += [(int(q), "lit", int(b[q])) for q in np.flatnonzero(literal)]
    return [(kind, value) for _, kind, value in sorted(found)]


def remainders(segment, D):
    """The lengths of the runs' last pieces (what is left after the pieces of 258), for tests that need 1 and 2 among them."""
    b = np.asarray(segment, np.uint8)
    rep = np.zeros(len(b), bool)
    rep[D:] = b[D:] == b[:-D]
    edges = np.flatnonzero(np.diff(np.concatenate(([0], rep.astype(np.int8), [0]))))
    return [int((end - start - 1) % 258 + 1) for start, end in zip(edges[::2], edges[1::2])]


class _Bits:
    def __init__(self, data, at):
        self.data, self.pos = data, at * 8

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lengths):
    """{(length, code): symbol} of a canonical Huffman code; raises ValueError unless it is complete (or has at most one code)."""
    count = np.bincount(np.asarray(lengths, np.int64), minlength=16)
    count[0] = 0
    kraft = sum(int(c) << (15 - l) for l, c in enumerate(count) if l)
    if kraft != 1 << 15 and int(count.sum()) > 1:
        raise ValueError(f"the code is not complete: Kraft sum {kraft} / 32768")
    code, first = 0, {}
    for l in range(1, 16):
        code = (code + int(count[l - 1])) << 1
        first[l] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(int(l), first[int(l)])] = sym
            first[int(l)] += 1
    return table


def _symbol(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        if (l, code) in table:
            return table[(l, code)]
    raise ValueError("no such code")


def parse(stream):
    """The blocks of a zlib stream: [{"type": "stored" | "dynamic", "final": bool, "tokens": [...], "bytes": n, "max_length": longest
    literal/length code, "max_cl_length": longest code-length code, "distance_lengths": [...]}], tokens as tokens() gives them, with
    ("match", length, distance). Stored blocks carry ("stored", n)."""
    data = bytes(stream)
    assert data[0] == 0x78 and (data[0] * 256 + data[1]) % 31 == 0
    bits, blocks = _Bits(data, 2), []
    while True:
        final, kind = bits.take(1), bits.take(2)
        if kind == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, inv = bits.take(16), bits.take(16)
            assert n ^ inv == 0xFFFF
            bits.pos += 8 * n
            blocks.append({"type": "stored", "final": bool(final), "tokens": [("stored", n)], "bytes": n})
        elif kind == 2:
            hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
            cl = [0] * 19
            for k in range(hclen):
                cl[CL_ORDER[k]] = bits.take(3)
            cl_table = _decoder(cl)
            lengths = []
            while len(lengths) < hlit + hdist:
                s = _symbol(bits, cl_table)
                if s < 16:
                    lengths.append(s)
                elif s == 16:
                    lengths += [lengths[-1]] * (3 + bits.take(2))
                else:
                    lengths += [0] * (3 + bits.take(3) if s == 17 else 11 + bits.take(7))
            assert len(lengths) == hlit + hdist
            lit, dist = _decoder(lengths[:hlit]), lengths[hlit:]
            dist_table = _decoder(dist) if any(dist) else {}
            toks, n = [], 0
            while True:
                s = _symbol(bits, lit)
                if s == 256:
                    break
                if s < 256:
                    toks.append(("lit", s))
                    n += 1
                else:
                    length = LENGTH_BASE[s - 257] + bits.take(LENGTH_EXTRA[s - 257])
                    d = _symbol(bits, dist_table)
                    toks.append(("match", length, DIST_BASE[d] + bits.take(DIST_EXTRA[d])))
                    n += length
            blocks.append({"type": "dynamic", "final": bool(final), "tokens": toks, "bytes": n, "max_length": max(lengths[:hlit]),
                           "max_cl_length": max(cl), "distance_lengths": dist})
        else:
            raise ValueError(f"block type {kind}")
        if final:
            break
    assert (bits.pos + 7) // 8 + 4 == len(data)
    return blocks


def huffman_depth(histogram):
    """The depth of the deepest leaf of the (unconstrained) Huffman tree of the non-zero counts."""
    heap = [(int(c), 0) for c in histogram if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def inflate(stream):
    """(the bytes, eof, unused) by zlib's own decoder."""
    d = zlib.decompressobj()
    out = d.decompress(bytes(stream))
    return out, d.eof, d.unused_data
