"""What the tests/test_*_abi.py files share: include/mscomp_amd.h read once, and the check that a feature's symbols are exported by the
library, named in api.EXPORTS and declared in the header."""
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mscomp_amd.h")


@functools.lru_cache(maxsize=None)
def header():
    """the header's text"""
    return open(HEADER).read()


@functools.lru_cache(maxsize=None)
def flat_header():
    """the header without comments, on one line, and without the gaps the comments leave in front of ',' and ')'"""
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header(), flags=re.S))
    return flat.replace(" ,", ",").replace(" )", ")")


def check_declared(lib, names, prototypes=()):
    """Every name is exported by ``lib``, listed in api.EXPORTS and declared in the header outside its comments; ``prototypes`` (one per
    name, in the names' order) are held to the flat header verbatim. Returns the header's text."""
    import ms_compress_amd as m
    assert len(prototypes) in (0, len(names))
    for s in names:
        assert hasattr(lib, s), "libmscomp_amd.so does not export " + s
        assert s in m.api.EXPORTS, s
        assert s + "(" in flat_header(), s + " is not declared in include/mscomp_amd.h"
    for s, proto in zip(names, prototypes):
        assert " " + s + "(" in proto and proto in flat_header(), s
    return header()
