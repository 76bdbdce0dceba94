"""CPU: the comparisons of tests/blocks_rig.py that the GPU tests of the block family rely on. Each gets a synthetic "device result" equal to
a small hand-written model answer -- one resource, two table rows, a dozen packed bytes, the guards -- which passes, and then one mutation
at a time, each of which must fail: a shared check that let one of them through would be laxer than the checks it replaced."""
import copy

import numpy as np
import pytest

import blocks_rig as G

PACKED = bytes(range(1, 13))
SLACK = 64


def new_model():
    return {"packed": PACKED, "first": np.array([0, 2], dtype=np.uint64), "off": np.array([0, 5, 12], dtype=np.uint64),
            "crc": np.array([0x11111111, 0x22222222], dtype=np.uint32), "new_len": [20], "status": [0]}


def new_got(crc=True):
    mo = new_model()
    image = np.full(len(PACKED) + SLACK, G.FILL, dtype=np.uint8)
    image[: len(PACKED)] = np.frombuffer(PACKED, dtype=np.uint8)
    return {"image": image, "first": mo["first"].copy(), "off": mo["off"].copy(),
            "crc": mo["crc"].copy() if crc else np.full(2, G.CRC_FILL, dtype=np.uint32), "new_len": [20], "status": [0]}


def poke(key, at, value):
    def change(got):
        got[key][at] = value
    return change


def grow_first(got):
    """(not a write a device could make -- d_first has exactly n + 1 entries --: it pins that the comparison is of whole arrays, lengths included)"""
    got["first"] = np.append(got["first"], np.uint64(2))


NEW_MUTATIONS = {
    "a packed byte": poke("image", 3, 0),
    "the byte behind the packed bytes": poke("image", len(PACKED), 0),
    "the last byte of the slack": poke("image", len(PACKED) + SLACK - 1, 0),
    "an offset": poke("off", 1, 6),
    "the last entry of first": poke("first", 1, 3),
    "an entry behind first's end": grow_first,
    "a status": poke("status", 0, -3),
    "a length": poke("new_len", 0, 21),
    "a checksum": poke("crc", 1, 0x22222223),
}


def test_same_image_names_the_first_differing_byte():
    got = new_got()["image"]
    G.same_image(got, PACKED, G.FILL, "image")
    G.same_image(got, [(0, PACKED[:5]), (5, PACKED[5:])], G.FILL, "image in two pieces")
    for at in (3, len(PACKED), len(got) - 1):
        bad = got.copy(); bad[at] ^= 0x01
        with pytest.raises(AssertionError) as e:
            G.same_image(bad, PACKED, G.FILL, "image")
        assert e.value.args[0][-1] == at
    with pytest.raises(AssertionError):
        G.same_image(got, PACKED, 0x00, "another fill")


def test_new_container_accepts_the_model_answer():
    G.NewContainer.compare(new_got(), new_model(), "new", 1, 2)
    G.NewContainer.compare(new_got(crc=False), new_model(), "new, checksums not asked for", 1, 2, crc=False)
    got = new_got(); got["crc"] = None                             # no checksum array at all
    G.NewContainer.compare(got, new_model(), "new, no checksum array", 1, 2, crc=False)
    mo = new_model(); mo["res_status"] = mo.pop("status")          # the statuses under the name a resize model gives them
    G.NewContainer.compare(new_got(), mo, "new", 1, 2, status="res_status")


@pytest.mark.parametrize("name", list(NEW_MUTATIONS))
def test_new_container_refuses(name):
    got = new_got()
    NEW_MUTATIONS[name](got)
    with pytest.raises(AssertionError):
        G.NewContainer.compare(got, new_model(), name, 1, 2)


def test_new_container_watches_a_checksum_array_that_was_not_asked_for():
    got = new_got(crc=False)
    got["crc"][1] = 0x22222222                                     # the model's own value: written all the same
    with pytest.raises(AssertionError):
        G.NewContainer.compare(got, new_model(), "crc fill", 1, 2, crc=False)
    with pytest.raises(AssertionError):                            # asked for, and left unwritten
        G.NewContainer.compare(new_got(crc=False), new_model(), "crc unwritten", 1, 2, crc=True)


def test_new_container_without_resources_keeps_its_one_entry_sentinels():
    mo = {"packed": b"", "first": np.array([0], dtype=np.uint64), "off": np.array([0], dtype=np.uint64), "crc": np.zeros(0, dtype=np.uint32),
          "new_len": [], "status": []}

    def got():
        return {"image": np.full(SLACK, G.FILL, dtype=np.uint8), "first": mo["first"].copy(), "off": mo["off"].copy(),
                "crc": np.full(1, G.CRC_FILL, dtype=np.uint32), "new_len": [G.M.M64], "status": [G.ST_FILL]}
    G.NewContainer.compare(got(), mo, "empty", 0, 0)
    for key, value in (("status", 0), ("new_len", 0), ("crc", 0)):
        bad = got(); bad[key][0] = value
        with pytest.raises(AssertionError):
            G.NewContainer.compare(bad, mo, "empty, %s written" % key, 0, 0)


def list_model():
    return {"rep": [0, 1], "ext_first": [0, 1, 1], "ext": [(0, 0, 0, 2)], "status": [0, -3]}


def list_got():
    s, g = G.SENT, G.ENTRY_GUARD
    return {"rep": [0, 1] + [s] * g, "ext_first": [0, 1, 1] + [s] * g, "ext": [0, 0, 0, 2] + [s] * (4 + g), "status": [0, -3] + [G.SENT32] * g}


def test_list_outs_accepts_the_model_answer():
    G.ListOuts.compare(list_got(), list_model(), exact=("rep", "ext_first"), prefixes=("ext",))


@pytest.mark.parametrize("key,at", [("rep", 2), ("rep", -1), ("ext_first", 3), ("ext_first", -1), ("status", 2), ("status", -1), ("ext", -1), ("ext", -G.ENTRY_GUARD),
                                    ("ext", 4), ("rep", 1), ("status", 1), ("ext", 3)],
                         ids=lambda v: str(v))
def test_list_outs_refuses_one_changed_entry(key, at):
    """a guard entry of every array, the first sentinel behind the extents in use, and an entry of the answer itself"""
    got = copy.deepcopy(list_got())
    got[key][at] = 9
    with pytest.raises(AssertionError):
        G.ListOuts.compare(got, list_model(), exact=("rep", "ext_first"), prefixes=("ext",))


def test_same_lists_is_list_outs_compare_in_numpy():
    """the closed-form comparison of the million-row tests: the answer, then one changed entry, one written guard and one written status"""
    torch = pytest.importorskip("torch")
    want = {"rep": [0, 1], "ext": [0, 0, 0, 2], "status": [0, -3]}

    def outs():
        o = G.ListOuts(torch.device("cpu"), {"rep": 2, "ext": 8}, 2)
        o["rep"][:2] = torch.tensor([0, 1]); o["ext"][:4] = torch.tensor([0, 0, 0, 2]); o.status[:2] = torch.tensor([0, -3], dtype=torch.int32)
        return o
    G.same_lists(outs(), want)
    for key, at in (("rep", 1), ("rep", 2), ("ext", 3), ("ext", 4), ("ext", -1), ("status", 1), ("status", -1)):
        o = outs()
        (o.status if key == "status" else o[key])[at] = 9
        with pytest.raises(AssertionError):
            G.same_lists(o, want)


def test_d64_pads_with_zeros_to_the_least_length():
    torch = pytest.importorskip("torch")
    cpu = torch.device("cpu")
    assert G.d64([], cpu).tolist() == [0] and G.d64([], cpu, 3).tolist() == [0, 0, 0]
    assert G.d64([5, 6], cpu).tolist() == [5, 6] and G.d64([5, 6], cpu, 4).tolist() == [5, 6, 0, 0]
    assert G.d64(np.array([[1, 2], [3, G.M.M64]], dtype=np.uint64), cpu).tolist() == [1, 2, 3, -1]


def test_memo_makes_once_per_key_and_closes():
    class Thing:
        closed = 0

        def close(self):
            Thing.closed += 1
    made = []
    gen = G.memo(lambda a, b: made.append((a, b)) or Thing())
    get = next(gen)
    assert get(1, 2) is get(1, 2) and get(1, 3) is not get(1, 2) and made == [(1, 2), (1, 3)]
    assert list(gen) == [] and Thing.closed == 2
    gen = G.memo()                                                 # the maker follows the key
    get = next(gen)
    assert get("k", 4096, lambda: [1]) is get("k", 4096, lambda: [2]) and get("k", 4096, lambda: [3]) == [1]
    assert list(gen) == []
