"""What the GPU tests of the parity object (tests/test_gpu_parity_rows.py) add to tests/blocks_rig.py and tests/repair_rig.py: one build
and one rebuild with sentinel-filled, guarded outputs compared with tests/parity_model.py array for array and image for image. torch is
imported inside the functions that need it. Not collected as a test."""
import numpy as np

import parity_model as Y
from blocks_rig import d64, i32, same_image, CAP_GUARD, ENTRY_GUARD, FILL, SENT, SENT32, ST_FILL

FILL32 = FILL * 0x01010101


def _full(dev, n, v, t):
    import torch
    return torch.full((n + ENTRY_GUARD,), v, dtype=t, device=dev)


def _u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def _u32(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint32)]


def _whole(got, want, guard, what):
    """an output array against the model's: its entries and nothing but sentinels behind them, or all sentinels where the call writes nothing"""
    want = [] if want is None else [int(x) for x in want]
    assert got == want + [guard] * (len(got) - len(want)), (what, got, want)


class ParitySet:
    """the outputs of a build for a table of nbt rows: d_par of ``room`` bytes of FILL with CAP_GUARD more behind them, and the five arrays"""

    def __init__(self, dev, nbt, k, m, room):
        import torch
        self.dev, self.nbt, self.k, self.m, self.room = dev, nbt, k, m, room
        self.Q = Y.geometry(nbt, k, m)[1]
        self.d_par = torch.full((room + CAP_GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.d_off, self.d_head = _full(dev, self.Q + 1, SENT, torch.int64), _full(dev, 4, SENT, torch.int64)
        self.d_crc, self.d_rl, self.d_st = _full(dev, self.Q, SENT32, torch.int32), _full(dev, nbt, SENT32, torch.int32), _full(dev, 1, ST_FILL, torch.int32)

    def reset(self):
        self.d_par.fill_(FILL); self.d_off.fill_(SENT); self.d_head.fill_(SENT); self.d_crc.fill_(SENT32); self.d_rl.fill_(SENT32); self.d_st.fill_(ST_FILL)

    def build(self, pr, view, par_cap=None):
        pr.build(view, self.d_par, self.d_off, self.d_crc, self.d_rl, self.d_head, self.d_st, par_cap=self.room if par_cap is None else par_cap)

    def against(self, mo, what):
        _whole(_u64(self.d_off), mo["par_off"], SENT, (what, "par_off"))
        _whole(_u32(self.d_crc), mo["par_crc"], SENT32, (what, "par_crc"))
        _whole(_u32(self.d_rl), mo["row_len"], SENT32, (what, "row_len"))
        _whole(_u64(self.d_head), mo["head"], SENT, (what, "par_head"))
        _whole([int(x) for x in self.d_st.cpu().numpy()], [mo["status"]], ST_FILL, (what, "status"))
        same_image(self.d_par.cpu().numpy(), mo["pieces"], FILL, (what, "d_par"))

    def damaged(self, par=(), crc=()):
        """a copy whose parity bytes at ``par`` and CRC words at ``crc`` are flipped, with the host set that says the same"""
        import copy
        c = copy.copy(self)
        c.d_par, c.d_crc = self.d_par.clone(), self.d_crc.clone()
        for at in par:
            c.d_par[at] ^= 0x40
        for q in crc:
            c.d_crc[q] ^= 0x1001
        return c

    def host(self, par_len):
        """the set as the model reads it"""
        return {"par": bytes(self.d_par.cpu().numpy()[:par_len]), "par_off": np.array(_u64(self.d_off)[: self.Q + 1], dtype=np.uint64),
                "par_crc": np.array(_u32(self.d_crc)[: self.Q], dtype=np.uint32), "row_len": np.array(_u32(self.d_rl)[: self.nbt], dtype=np.uint32),
                "head": np.array(_u64(self.d_head)[:4], dtype=np.uint64)}


def check_build(pr, con, pset=None, par_cap=None, nbt=None, what="build"):
    """one BlockParity.build over the Container ``con`` compared with the model; returns (model, ParitySet)"""
    room = pr.bound()[1]
    pset = pset or ParitySet(con.dev, pr.n_blocks_table, pr.k, pr.m, room)
    pset.reset()
    pset.build(pr, con.view(False, nbt=nbt), par_cap)
    con.ctx.stream.synchronize()
    mo = Y.model_build(con.model(False, nbt=nbt), con.B, pr.k, pr.m, room if par_cap is None else par_cap, nbt=pr.n_blocks_table)
    pset.against(mo, what)
    return mo, pset


class FixOuts:
    """the outputs of a rebuild: d_fix of ``room`` bytes of FILL with CAP_GUARD more behind them, and the four arrays"""

    def __init__(self, dev, nbt, room):
        import torch
        self.dev, self.nbt, self.room = dev, nbt, room
        self.d_fix = torch.full((room + CAP_GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.d_off, self.d_count = _full(dev, nbt + 1, SENT, torch.int64), _full(dev, 6, SENT, torch.int64)
        self.d_ver, self.d_st = _full(dev, nbt, SENT32, torch.int32), _full(dev, 1, ST_FILL, torch.int32)

    def reset(self):
        self.d_fix.fill_(FILL); self.d_off.fill_(SENT); self.d_count.fill_(SENT); self.d_ver.fill_(SENT32); self.d_st.fill_(ST_FILL)

    def rebuild(self, pr, view, d_verdict, pset, par_len, fix_cap=None):
        pr.rebuild(view, d_verdict, pset.d_par, pset.d_off, pset.d_crc, pset.d_rl, pset.d_head, self.d_fix, self.d_off, self.d_ver, self.d_count, self.d_st,
                   par_len=par_len, fix_cap=self.room if fix_cap is None else fix_cap)

    def against(self, mo, what):
        _whole(_u64(self.d_off), mo["fix_off"], SENT, (what, "fix_off"))
        _whole(_u32(self.d_ver), mo["fix_verdict"], SENT32, (what, "fix_verdict"))
        _whole(_u64(self.d_count), mo["count"], SENT, (what, "count"))
        _whole([int(x) for x in self.d_st.cpu().numpy()], [mo["status"]], ST_FILL, (what, "status"))
        same_image(self.d_fix.cpu().numpy(), mo["pieces"], FILL, (what, "d_fix"))


def check_rebuild(pr, con, verdict, pset, par_len, outs=None, fix_cap=None, nbt=None, d_verdict=None, what="rebuild"):
    """one BlockParity.rebuild over the (damaged) Container ``con``, its verdicts and the ParitySet compared with the model; returns
    (model, FixOuts)"""
    outs = outs or FixOuts(con.dev, pr.n_blocks_table, con.plen + 64)
    outs.reset()
    d_verdict = i32(np.asarray(verdict, dtype=np.uint32), con.dev) if d_verdict is None else d_verdict
    outs.rebuild(pr, con.view(False, nbt=nbt), d_verdict, pset, par_len, fix_cap)
    con.ctx.stream.synchronize()
    mo = Y.model_rebuild(con.model(False, nbt=nbt), verdict, pset.host(par_len), con.B, pr.k, pr.m, outs.room if fix_cap is None else fix_cap, nbt=pr.n_blocks_table,
                         par_len=par_len)
    outs.against(mo, what)
    return mo, outs


def fix_container(con, outs, mo):
    """the sparse mirror as a Container beside ``con``: the fix's stored bytes and offsets, the primary's first, lens and crc"""
    c = con.edited(off=np.array(mo["fix_off"], dtype=np.uint64))
    c.d_packed, c.d_boff = outs.d_fix, outs.d_off
    c.plen = c.cap = int(mo["fix_off"][-1])
    image = bytearray(c.plen)
    for at, b in mo["pieces"]:
        image[at: at + len(b)] = b
    c.packed = bytes(image)
    return c
