"""What the GPU tests of salvage and repair (tests/test_gpu_repair.py) add to tests/blocks_rig.py: one salvage call with sentinel-filled,
guarded outputs compared with tests/repair_model.py array for array and image for image (check_salvage), one repair call compared the same
way (check_repair), and the splice the header's consequence speaks of, run from the call's own device arrays (rebuild). torch is imported
inside the functions that need it. Not collected as a test."""
import numpy as np

import repair_model as P
from blocks_rig import ListOuts, Spliced, d64, i32, same_image, ENTRY_GUARD, FILL, SENT, SENT32, ST_FILL

REPAIR_EXACT, REPAIR_PREFIXES = ("ext_first", "fixed", "lost", "count"), ("ext",)


def damaged(healthy, edits):
    """the copy of a healthy Container that states a recipe's edits"""
    return healthy.edited(**{k: v for k, v in edits.items() if k != "caps"})


class SalvageOuts:
    """the outputs of a salvage of n resources over nbmax rows: d_out of ``room`` bytes of FILL, and the six arrays sentinel-filled with
    ENTRY_GUARD entries behind each"""

    def __init__(self, dev, n, nbmax, room):
        import torch
        self.n, self.nbmax = n, nbmax
        full = lambda k, v, t: torch.full((k + ENTRY_GUARD,), v, dtype=t, device=dev)
        self.d_out = torch.full((room,), FILL, dtype=torch.uint8, device=dev)
        self.d_olen, self.d_count = full(n, SENT, torch.int64), full(4, SENT, torch.int64)
        self.d_bad, self.d_verdict, self.d_st = full(n, SENT32, torch.int32), full(nbmax, SENT32, torch.int32), full(n, ST_FILL, torch.int32)

    def reset(self):
        self.d_out.fill_(FILL); self.d_olen.fill_(SENT); self.d_count.fill_(SENT)
        self.d_bad.fill_(SENT32); self.d_verdict.fill_(SENT32); self.d_st.fill_(ST_FILL)

    def pull(self):
        u64 = lambda t: [int(x) for x in t.cpu().numpy().view(np.uint64)]
        i = lambda t: [int(x) for x in t.cpu().numpy()]
        return {"image": self.d_out.cpu().numpy(), "out_len": u64(self.d_olen), "count": u64(self.d_count), "bad": i(self.d_bad),
                "verdict": i(self.d_verdict), "status": i(self.d_st)}

    def against(self, mo, out_off, B, what):
        """everything the call wrote, and everything it must not have written, against the model"""
        got = self.pull()
        for key, guard in (("verdict", SENT32), ("bad", SENT32), ("status", ST_FILL), ("out_len", SENT), ("count", SENT)):
            want = [int(x) for x in mo[key]]
            assert got[key] == want + [guard] * ENTRY_GUARD, (what, key, got[key], want)
        same_image(got["image"], P.image_pieces(mo, out_off, B), FILL, (what, "d_out"))
        return got


def salvage(healthy, con, outs, out_off, caps, crc=True, d_only=None, bk=None):
    """one BlockContainer.salvage of ``con`` (a copy of ``healthy``, damaged or not) through the healthy container's BlockContainer"""
    dev = healthy.dev
    (bk or healthy.bk).salvage(con.d_packed, con.d_first, con.d_boff, con.d_len, outs.d_out, d64(out_off, dev), d64(caps, dev), outs.d_olen, outs.d_bad,
                               outs.d_verdict, outs.d_count, outs.d_st, d_block_crc=con.d_crc if crc else None, d_only=d_only, packed_len=con.cap)


def check_salvage(oracle, healthy, con, caps=None, crc=True, only=None, residues=None, what="salvage", outs=None):
    """run, and compare with the model; returns (model, SalvageOuts, output offsets)"""
    caps = list(con.lens) if caps is None else caps
    out_off, room = healthy.layout(caps, residues)
    outs = outs or SalvageOuts(healthy.dev, healthy.n, healthy.nbt, room)
    outs.reset()
    d_only = None if only is None else i32(np.asarray(only, dtype=np.uint32), healthy.dev)
    salvage(healthy, con, outs, out_off, caps, crc, d_only)
    healthy.ctx.stream.synchronize()
    mo = P.model_salvage(oracle, healthy.fmt, con.model(), healthy.B, healthy.total, caps, with_crc=crc, only=only)
    outs.against(mo, out_off, healthy.B, what)
    return mo, outs, out_off


def repair_outs(dev, n, room):
    """the six output arrays of a repair of n resources within ``room`` rows, sentinel-filled and guarded"""
    outs = ListOuts(dev, {"ext_first": n + 1, "ext": 4 * room, "fixed": n, "lost": n, "count": 4}, n)
    outs.n, outs.room = n, room
    return outs


def check_repair(srcs, verdicts, n=None, room=None, with_crc=True, dd=None, outs=None, d_verdicts=None):
    """one BlockDeduper.repair over the Containers ``srcs`` (the primary first) and their verdict arrays compared with the model, entry for
    entry; returns (model, ListOuts)"""
    import ms_compress_amd as m
    p = srcs[0]
    n = p.n if n is None else n
    room = int(p.first[-1]) if room is None else room
    deduper = dd or m.BlockDeduper.for_repair(p.ctx, p.B, len(srcs), n, room)
    outs = outs or repair_outs(p.dev, n, room)
    outs.reset()
    d_verdicts = d_verdicts or [i32(np.asarray(v, dtype=np.uint32), p.dev) for v in verdicts]
    deduper.repair([s.view(with_crc) for s in srcs], d_verdicts, *outs.tensors())
    p.ctx.stream.synchronize()
    if dd is None:
        deduper.close()
    mo = P.model_repair([s.model(with_crc) for s in srcs], verdicts, p.B, n, room, with_crc)
    outs.against(mo, exact=REPAIR_EXACT, prefixes=REPAIR_PREFIXES)
    return mo, outs


def rebuild(srcs, mo, outs, with_crc=True, healthy=None, built=None, sp=None):
    """the header's consequence on the GPU, from the device arrays the repair left: the splice by extents over the same views, held to the
    extents model, and -- with ``healthy`` and nothing lost -- byte for byte to the undamaged container"""
    import ms_compress_amd as m
    p = srcs[0]
    cap = sum(s.cap for s in srcs) + 32
    built = built or Spliced(p.dev, outs.n, p.nbt, cap, with_crc)
    splicer = sp or m.BlockSplicer.for_extents(p.ctx, p.B, len(srcs), outs.n, outs.room, p.nbt)
    built.run(splicer, [s.view(with_crc) for s in srcs], outs["ext_first"], outs["ext"])
    p.ctx.stream.synchronize()
    if sp is None:
        splicer.close()
    mb = P.model_rebuild([s.model(with_crc) for s in srcs], mo, p.B, with_crc, n_ext=outs.room, cap=built.room)
    built.against(mb, "rebuilt", crc=with_crc)
    if healthy is not None and not any(mo["status"]):
        got = built.as_built()
        assert bytes(got["packed"][: healthy.plen]) == healthy.packed and int(got["off"][int(got["first"][-1])]) == healthy.plen
        assert np.array_equal(got["first"], healthy.first) and np.array_equal(got["off"], healthy.off) and got["new_len"] == healthy.lens
        assert not with_crc or np.array_equal(got["crc"], healthy.crc)
    return mb, built
