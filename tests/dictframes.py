"""Hand-built frames that name a dictionary (test helper, no tests): a frame header with a 4-byte Dictionary_ID in front of blocks made byte
by byte, so that a frame's FIRST sequences reach exactly where a dictionary's content begins or ends, or take their offset from the
dictionary's offset history. tests/seqframes.py cannot make these: libzstd's ZSTD_compressSequences refuses an offset beyond what the frame
has produced, and it writes no Dictionary_ID. The oracle (with the dictionary registered) says what each frame decodes to."""
from test_exact_cpu import lit_block, raw_block   # noqa: F401  (re-exported: blocks without sequences)

WINDOW_LOG = 17


def header(dict_id, window_log=WINDOW_LOG):
    """magic, descriptor 0x03 (4-byte Dictionary_ID, no content size, no checksum), window descriptor, the id"""
    return bytes([0x28, 0xB5, 0x2F, 0xFD, 0x03, (window_log - 10) << 3]) + dict_id.to_bytes(4, "little")


def seq_block_value(value, lits=b"abcd", last=False):
    """compressed block: raw literals, ONE sequence with literal length 0 and match length 3 whose offset VALUE is given (1, 2, 3: the repeat
    codes — with a literal length of 0 they name history[1], history[2] and history[0] - 1; value >= 4: the offset value - 3), LL / ML
    predefined (state 0: length code 0), OF in RLE mode. The literals follow the match."""
    assert value >= 1 and len(lits) < 32
    of_code = value.bit_length() - 1
    extra = value - (1 << of_code)
    acc, accn = 1, 1
    for v, w in ((0, 6), (0, 6), (extra, of_code)):       # top-down: marker, LL state, (OF state: 0 bits), ML state, extra bits of OF
        acc = (acc << w) | (v & ((1 << w) - 1))
        accn += w
    stream = acc.to_bytes((accn + 7) // 8, "little")
    body = bytes([len(lits) << 3]) + lits + bytes([1, 0x10, of_code]) + stream
    return (((len(body) << 3) | (2 << 1) | (1 if last else 0)).to_bytes(3, "little")) + body


def seq_block(offset, lits=b"abcd", last=False):
    return seq_block_value(offset + 3, lits, last)


def frame(dict_id, *blocks):
    return header(dict_id) + b"".join(blocks)


def patch_dict_id(z, new_id):
    """the same frame naming another dictionary: the 4-byte Dictionary_ID field rewritten in place (same field width)"""
    assert z[:4] == bytes([0x28, 0xB5, 0x2F, 0xFD]) and z[4] & 3 == 3
    at = 5 + (0 if (z[4] >> 5) & 1 else 1)
    return z[:at] + new_id.to_bytes(4, "little") + z[at + 4:]


def first_block(z):
    """(block type, literals type, sequence modes byte or None) of a frame's first block, from its headers"""
    d = z[4]
    at = 5 + (0 if (d >> 5) & 1 else 1) + (0, 1, 2, 4)[d & 3]
    fcs = d >> 6
    at += (1 if (d >> 5) & 1 else 0) if fcs == 0 else (2, 4, 8)[fcs - 1]
    bh = int.from_bytes(z[at:at + 3], "little")
    btype, body = (bh >> 1) & 3, at + 3
    if btype != 2:
        return btype, None, None
    lt, sf = z[body] & 3, (z[body] >> 2) & 3
    if lt < 2:
        hl = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = z[body] >> 3 if sf in (0, 2) else (int.from_bytes(z[body:body + 2], "little") >> 4 if sf == 1 else int.from_bytes(z[body:body + 3], "little") >> 4)
        seq = body + hl + (regen if lt == 0 else 1)
    else:
        hl = (3, 3, 4, 5)[sf]
        v = int.from_bytes(z[body:body + hl], "little") >> 4
        bits = (10, 10, 14, 18)[sf]
        seq = body + hl + (v >> bits)
    n0 = z[seq]
    if n0 == 0:
        return btype, lt, None
    modes = z[seq + 1] if n0 < 128 else z[seq + 2] if n0 < 255 else z[seq + 3]
    return btype, lt, modes
