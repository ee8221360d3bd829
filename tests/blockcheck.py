"""The per-block intermediates of a decode against the oracle's (test helper, no tests): Huffman tables and literals, FSE tables,
sequences (actual offset, match length, match destination, literal start) and the offset history at every block start. Shared by
the CPU harness tests (emu.EmuBatch) and the GPU tests (zgpu.Batch)."""
import oracle

_KEYS = ("btype", "status", "lit_type", "regen_size", "nseq", "huf_slot", "ll_slot", "of_slot", "ml_slot")


def oracle_blocks(z):
    """decode the frame at the start of z block by block with the oracle, collecting its intermediates"""
    d = oracle.FrameDecoder()
    d.set_max_window_size(1 << 31)
    st, c, _, _ = d.init(z)
    assert st == 0
    pos, blocks = c, []
    while not d.is_finished():
        st, used, fin = d.decode_blocks(z[pos:], oracle.STRAT_UPTO_BLOCKS, 1)
        assert st == 0
        pos += used
        rec = {"type": d.last_block_type(), "hist_after": d.offset_hist()}
        if rec["type"] == 2:
            rec["literals"] = d.last_literals()
            rec["sequences"] = d.last_sequences()
            rec["huf"] = d.huf_table()
            rec["fse"] = [d.fse_table(k) for k in range(3)]
        blocks.append(rec)
        if fin:
            break
    return blocks


def _block(src, b):
    """(info dict, offset history at the block's start) from an emu.EmuBatch or a zgpu.Batch"""
    if hasattr(src, "block_info"):
        i = src.block_info(b)
        return {k: getattr(i, k) for k in _KEYS}, list(i.hist_init)
    return src.block(b), src.block_hist(b)


def check_frame(src, first_block, ob, where):
    """compare blocks first_block .. first_block + len(ob) - 1 of src with the oracle's records ob (oracle_blocks) of that frame"""
    hist = [1, 4, 8]
    for j, rec in enumerate(ob):
        b = first_block + j
        info, h = _block(src, b)
        assert info["btype"] == rec["type"] and info["status"] == 0, (where, j, info)
        assert h == hist, (where, j, h, hist)
        hist = rec["hist_after"]
        if rec["type"] != 2:
            continue
        if info["lit_type"] >= 2:       # Huffman literals: bytes and the table they were decoded with
            assert src.block_literals(b, info["regen_size"]) == rec["literals"], (where, j)
            tab, mb = src.huf_slot(info["huf_slot"])
            oents, omb = rec["huf"]
            assert mb == omb, (where, j)
            assert [(tab[i] & 255, tab[i] >> 8) for i in range(1 << mb)] == oents, (where, j)
        seqs = src.block_sequences(b, info["nseq"])
        oseq = rec["sequences"]
        assert len(oseq) == info["nseq"] == len(seqs), (where, j)
        # a zgpu.Batch returns the two position fields of its ZgSeq records, which hold 17 bits (zg_types.h): the same number for a block
        # of up to 128 KiB; for a larger one the positions mod 2^17, which with the exact ml and lit_start 0 at the block's start
        # still fix every ll (< 2^17) and so every position. The harness keeps 32-bit fields.
        mask = 0x1FFFF if hasattr(src, "block_info") else -1
        lit_pos = out_pos = 0
        for i, ((of, ml, mdst, lit_start), (oll, oml, _oof, oactual)) in enumerate(zip(seqs, oseq)):
            tag, k = of >> 30, of & 0x3FFFFFFF
            actual = of if tag == 0 else max(h[tag - 1] - k, 0)
            assert (actual, ml, mdst, lit_start) == (oactual, oml, (out_pos + oll) & mask, lit_pos & mask), (where, j, i)
            lit_pos += oll
            out_pos += oll + oml
        if info["nseq"]:                # the three FSE tables this block decoded with
            for k, slot in enumerate((info["ll_slot"], info["of_slot"], info["ml_slot"])):
                oents, olog, orle = rec["fse"][k]
                p, logs = src.fse_slot(slot)
                off = (0, 1024, 512)[k]
                if orle >= 0:
                    assert logs[k] == 0 and ((p[off] >> 20) & 63) == orle, (where, j, k)
                else:
                    assert logs[k] == olog, (where, j, k)
                    got = [(p[off + i] & 0xFFFF, (p[off + i] >> 16) & 15, (p[off + i] >> 20) & 63) for i in range(1 << olog)]
                    assert got == oents, (where, j, k)
    return len(ob)
