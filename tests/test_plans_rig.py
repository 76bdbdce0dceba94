"""CPU: the comparisons of tests/plans_rig.py that the GPU tests of the plan family rely on. A hand-written batch of three units (capacities
5, 0 and 9) gets a synthetic host result and a synthetic "device result" equal to it, which pass, and then one mutation at a time, each
of which must fail: a shared check that let one of them through would be laxer than the checks it replaced. The layout itself is checked
too."""
import numpy as np
import pytest

import plans_rig as PR

UNITS = [b"abc", b"", b"0123456789"]
CAPS = [5, 0, 9]
LENS, STS, NEEDS = [4, 0, 7], [0, 0, 0], [4, 0, 8]
SLACK = 32                                                           # bytes of the device buffer behind out_total


def batch():
    return PR.layout(UNITS, CAPS)


def result(b, slack=0, need=False):
    """units 0 and 2 wrote LENS bytes, and unit 2 two more behind its length (an uncounted terminator)"""
    out = np.full(b.out_total + slack, PR.GUARD, np.uint8)
    for i, n in enumerate(LENS):
        out[int(b.out_off[i]): int(b.out_off[i]) + n] = np.arange(1, n + 1, dtype=np.uint8) + 16 * i
    out[int(b.out_off[2]) + 7: int(b.out_off[2]) + 9] = 0
    res = (np.array(LENS, np.int64), np.array(STS, np.int32), out)
    return res + ((np.array(NEEDS, np.int64),) if need else ())


def poke(k, at, value):
    def change(res, b):
        res[k][at(b) if callable(at) else at] = value
    return change


MUTATIONS = {                                                        # name: (change, fails with tail=0 too)
    "a status": (poke(1, 2, -5), True),
    "a length": (poke(0, 0, 3), True),
    "a byte inside a unit's length": (poke(2, lambda b: int(b.out_off[2]) + 6, 0x99), True),
    "a byte in the two bytes behind the length": (poke(2, lambda b: int(b.out_off[2]) + 8, 0x99), False),
    "a byte in the gap in front of the first capacity": (poke(2, lambda b: int(b.out_off[0]) - 1, 0), True),
    "the first byte of the buffer": (poke(2, 0, 0), True),
    "a byte in the gap between two capacities": (poke(2, lambda b: int(b.out_off[0]) + 5, 0), True),
    "a byte at the offset of the unit without capacity": (poke(2, lambda b: int(b.out_off[1]), 0), True),
    "a byte in the gap behind the last capacity": (poke(2, lambda b: int(b.out_off[2]) + 9, 0), True),
    "the last byte before out_total": (poke(2, lambda b: b.out_total - 1, 0), True),
    "a byte past out_total": (poke(2, lambda b: b.out_total, 0), True),
    "the last byte of the buffer": (poke(2, -1, 0), True),
}


def test_same_accepts_an_equal_result():
    b = batch()
    for tail in (0, 2):
        PR.same(result(b), result(b, SLACK), b, tail=tail)
        PR.same(result(b), result(b, SLACK), b, [True, True, True], tail=tail)
    for res in (result(b), result(b, SLACK)):
        PR.guards_intact(res, b)
    assert PR.unit(result(b), b, 0) == bytes([1, 2, 3, 4]) and PR.unit(result(b), b, 1) == b""
    assert PR.unit(result(b), b, 2) == bytes(range(33, 40))


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_same_refuses(name):
    b = batch()
    change, without_tail = MUTATIONS[name]
    dev = result(b, SLACK)
    change(dev, b)
    with pytest.raises(AssertionError):
        PR.same(result(b), dev, b, tail=2)
    if without_tail:
        with pytest.raises(AssertionError):
            PR.same(result(b), dev, b)
    else:
        PR.same(result(b), dev, b)


@pytest.mark.parametrize("name", [k for k in MUTATIONS if "gap" in k or "buffer" in k or "out_total" in k or "without capacity" in k])
def test_guards_intact_refuses(name):
    b = batch()
    res = result(b, SLACK)
    MUTATIONS[name][0](res, b)
    with pytest.raises(AssertionError):
        PR.guards_intact(res, b)


def rejected(b):
    """unit 2 outside the accepted ones: (ARG, 0), its capacity untouched"""
    dev = result(b, SLACK)
    dev[0][2], dev[1][2] = 0, PR.ARG
    dev[2][int(b.out_off[2]): int(b.out_off[2]) + 9] = PR.GUARD
    return dev


def test_same_with_a_rejected_unit():
    b = batch()
    acc = [True, True, False]
    PR.same(result(b), rejected(b), b, acc, tail=2)
    for k, value in ((0, 7), (1, 0), (1, -5)):                        # a length, the status MSCOMP_OK, another status
        dev = rejected(b)
        dev[k][2] = value
        with pytest.raises(AssertionError):
            PR.same(result(b), dev, b, acc, tail=2)
    dev = rejected(b)                                                 # a byte written into the rejected unit's capacity
    dev[2][int(b.out_off[2]) + 3] = 0
    with pytest.raises(AssertionError):
        PR.same(result(b), dev, b, acc, tail=2)
    with pytest.raises(AssertionError):                               # and the rejection itself is no host plan's answer
        PR.same(result(b), rejected(b), b, tail=2)


def test_same_sizes():
    b = batch()
    PR.same_sizes(result(b, need=True), result(b, need=True))
    for k, at, value in ((1, 0, -3), (0, 2, 8), (3, 2, 7), (3, 1, 1)):     # a status, a length, two needs
        dev = result(b, need=True)
        dev[k][at] = value
        with pytest.raises(AssertionError):
            PR.same_sizes(result(b, need=True), dev)
    acc = [True, False, True]
    dev = result(b, need=True)
    dev[1][1] = PR.ARG
    PR.same_sizes(result(b, need=True), dev, acc)
    for k, value in ((0, 1), (3, 1), (1, 0)):                         # a rejected unit with a length, a need, the status MSCOMP_OK
        bad = tuple(a.copy() for a in dev)
        bad[k][1] = value
        with pytest.raises(AssertionError):
            PR.same_sizes(result(b, need=True), bad, acc)
    with pytest.raises(AssertionError):                               # a result of another unit count
        PR.same_sizes(result(b, need=True), tuple(a[:2] for a in result(b, need=True)))


@pytest.mark.parametrize("fill,dtype", [(PR.G_LEN, np.int64), (PR.G_ST, np.int32)])
def test_strip_guards(fill, dtype):
    n = 3
    a = np.full(n + 2 * PR.PAD, fill, dtype)
    a[PR.PAD: PR.PAD + n] = [4, 0, 7]
    assert PR.strip_guards(a, n, fill).tolist() == [4, 0, 7]
    assert len(PR.strip_guards(np.full(2 * PR.PAD, fill, dtype), 0, fill)) == 0
    for at in (0, PR.PAD - 1, PR.PAD + n, len(a) - 1):              # the first and last guard entry in front and behind
        bad = a.copy()
        bad[at] = 0
        with pytest.raises(AssertionError):
            PR.strip_guards(bad, n, fill)
    with pytest.raises(AssertionError):
        PR.strip_guards(a, n + 1, fill)


def test_layout():
    b = batch()
    blob, in_off, lens, out_off, caps, out_total = b                  # unpacks as the six fields
    assert lens.tolist() == [3, 0, 10] and caps.tolist() == CAPS and in_off.tolist() == [0, 16, 16]
    assert len(blob) == 32 + 16 and bytes(blob[:3]) == b"abc" and bytes(blob[16:26]) == UNITS[2] and not blob[26:].any()
    assert all(x.dtype == np.uint64 for x in (in_off, lens, out_off, caps))
    assert out_off[0] >= PR.GAP
    for i in range(2):                                              # ascending, GAP guard positions behind every capacity
        assert int(out_off[i + 1]) >= int(out_off[i]) + CAPS[i] + PR.GAP
    assert len(set(out_off.tolist())) == 3                          # the unit without capacity has an offset of its own
    assert out_total >= int(out_off[2]) + CAPS[2] + PR.GAP
    free = PR.layout(UNITS)                                          # no capacities: a size plan without limits
    assert free.caps is None and free.lens.tolist() == [3, 0, 10] and (free.blob == blob).all()
    assert PR.layout([], []).out_total >= PR.GAP and len(PR.layout([], []).blob) == 16
