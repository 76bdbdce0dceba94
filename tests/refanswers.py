"""What the compiled reference answers, for the tests that compare against it.

Where oracle/_ref was built (oracle/Makefile, from the reference's sources) every answer is computed live; everywhere else it is read from
tests/golden/ref_answers.json, which tools/make_golden_ref.py records from that same build. Both ways a test gets the same thing: the
digest of the reference's result, to be compared with ``digest`` of its own. A question is a tuple (kind, arguments...); its key is the
digest of the question itself, so a recorded answer is found by what was asked, not by the order of the calls.
"""
import hashlib
import json
import os

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_answers.json")
_recorded = None
live_answers = {}          # every answer computed live in this process: what tools/make_golden_ref.py writes out


def digest(x):
    """64-bit digest of repr(x) (byte strings, ints, tuples and lists of them)"""
    return hashlib.sha256(repr(x).encode()).hexdigest()[:16]


def answer(question, live):
    """digest of the reference's result for `question`. live: a callable that asks the compiled reference, or None where it was not built."""
    global _recorded
    key = digest(question)
    if live is not None:
        live_answers[key] = digest(live())
        return live_answers[key]
    if _recorded is None:
        with open(PATH) as f:
            _recorded = json.load(f)["answers"]
    if key not in _recorded:
        raise KeyError("no recorded answer of the reference for %r (tools/make_golden_ref.py records them)" % (question[:1],))
    return _recorded[key]


def record(path=PATH):
    """write the answers computed live so far, merged with those already in the file"""
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)["answers"]
    old.update(live_answers)
    with open(path, "w") as f:
        json.dump({"about": "digests of the compiled reference's answers (tests/refanswers.py; tools/make_golden_ref.py)",
                   "answers": dict(sorted(old.items()))}, f, indent=0, separators=(",", ":"))
        f.write("\n")
