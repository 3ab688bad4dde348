"""CPU: every behaviour switch of libpq_hip.so (the kOptions table, pq_api.hip) is named by at least one GPU test — or sits in EXEMPT below with a reason.

The header and pq_common.h promise of most switches "time only, never bits"; the A/B tools under tools/ measure with them and the planners' defaults were chosen from
those measurements.  A switch nobody launches under the suite is compiled device code (or launch geometry) that has never executed there, so a new switch needs a GPU test
that names it.  The second test ties the table of tests/test_gpu_switch_paths.py to the kernel trace recorded on an MI355X (profiles/r21_switch_paths_kernels.txt):
every kernel a row says it reaches was really launched by the three switch / rotation / grouped files."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# switch -> why no GPU test needs to name it
EXEMPT: dict = {}


def _option_names():
    src = open(os.path.join(ROOT, "protoquant_amd", "csrc", "pq_api.hip")).read()
    m = re.search(r"kOptions\[\]\s*=\s*\{(.*?)\n\};", src, re.S)
    assert m, "the kOptions table was not found in pq_api.hip"
    names = re.findall(r'^\s*\{"(PQ_[A-Z0-9_]+)",', m.group(1), re.M)
    assert len(names) >= 30 and len(set(names)) == len(names), names
    return names


def _gpu_test_sources():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))) + [os.path.join(ROOT, "tests", "fuzz_quant.py")]
    return {os.path.basename(f): open(f).read() for f in files}


def test_every_switch_is_named_by_a_gpu_test():
    srcs = _gpu_test_sources()
    missing = [n for n in _option_names() if n not in EXEMPT and not any(re.search(r"\b" + n + r"\b", s) for s in srcs.values())]
    assert not missing, f"switches that no tests/test_gpu_*.py names (add a bit-exact GPU test, or an EXEMPT entry with a reason): {missing}"
    stale = [n for n in EXEMPT if n not in _option_names()]
    assert not stale, f"EXEMPT names switches that no longer exist: {stale}"
    for n, why in EXEMPT.items():
        assert isinstance(why, str) and len(why) > 20, f"EXEMPT[{n}] needs a written reason"


def test_the_library_knows_exactly_the_table_names():
    """The environment pass and pq_set_option walk ONE table, so a switch cannot be known to one and not the other; what is left to hold is that the names this guard
    reads from the source are the names the built library answers to: each is accepted, an unknown one is refused by name, and they are unique and at least 30."""
    from protoquant_amd import _lib
    L = _lib.lib()
    names = _option_names()
    assert len(names) >= 30 and len(set(names)) == len(names), names
    for n in names:
        assert L.pq_set_option(n.encode(), b"") == 0, (n, L.pq_last_error())      # PQ_OK; "" restores the default
    for bogus in ("PQ_NO_SUCH_SWITCH", names[0] + "_", names[0][:-1], ""):
        assert L.pq_set_option(bogus.encode(), b"") == 1, bogus                   # PQ_ERR_BAD_ARG
        assert b"unknown option" in L.pq_last_error(), L.pq_last_error()


def _traced_kernels():
    path = os.path.join(ROOT, "profiles", "r21_switch_paths_kernels.txt")
    return [l.split(None, 1)[1].strip() for l in open(path) if l.strip() and not l.startswith("#")]


def test_switch_table_kernels_were_seen_in_the_recorded_trace():
    """tests/test_gpu_switch_paths.py imports without a GPU: its rows carry the fragment of the kernel name each one expects, and the trace of the three files on an
    MI355X lists that kernel.  Bits alone cannot tell a switched path from the default one that quietly ran instead."""
    from tests import test_gpu_switch_paths as T
    names = _traced_kernels()
    assert len(names) > 40
    frags = sorted({f for row in T.TABLE for f in row.kernels} | set(T.ALSO_TRACED))
    assert len(frags) >= 25
    unseen = [f for f in frags if not any(f in n for n in names)]
    assert not unseen, f"kernel name fragments that the recorded trace does not hold: {unseen}"
