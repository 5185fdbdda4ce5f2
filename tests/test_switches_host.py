"""The environment switches are declared once (emagls_amd/csrc/switches.hpp), documented once and set by
name from the tests and tools: this test reads the three as text and holds them together.  It looks for EMAGLS_ names only -- it
loads no library and compiles nothing."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "emagls_amd", "csrc")

# forms that were measured, lost and removed together with their switches (DESIGN_HISTORY.md, profiles/)
RETIRED = ["EMAGLS_CHOL_FUSED", "EMAGLS_JACOBI_PAIR", "EMAGLS_BACK_LDS", "EMAGLS_EAGER_SIDES", "EMAGLS_SLAB_FILL", "EMAGLS_JOBS_SHARED_STREAM",
           "EMAGLS_ATF_ONE_STREAM", "EMAGLS_SWEEP_SERIAL", "EMAGLS_SWEEP_REG_MIN", "EMAGLS_BENCH_FORK"]
# names only tests and tools use among themselves (never read by the library, not worth a row in section 8)
TEST_ONLY = re.compile(r"EMAGLS_(HRIR_FILE|HRIR_NPZ|LIBHDF5|RECORD_DECODE_PUSH_ERRORS|FUZZ_\w+|PMC_\w+|BUILD_TAG)$")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top, skip=()):
    for d, dirs, names in os.walk(top):
        dirs[:] = [x for x in dirs if x != "__pycache__" and os.path.join(d, x) not in skip]
        for n in names:
            yield os.path.join(d, n)


def _table_names():
    return {"EMAGLS_" + n for n in re.findall(r"^\s*X\((\w+),", _read(os.path.join(CSRC, "switches.hpp")), re.M)}


def _section8():
    """(names of the library table, names of the table of what the library does not read)"""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    sec = text[text.index("\n## 8. Environment switches"):text.index("\n## 9. ")]
    lib, other = sec.split("Not read by the library:")
    first_cell = lambda part: set(re.findall(r"EMAGLS_\w+", " ".join(re.findall(r"^\| (`EMAGLS_[^|]*)\|", part, re.M))))
    return first_cell(lib), first_cell(other)


def test_one_reader_of_the_environment():
    hits = [os.path.relpath(p, ROOT) for p in _files(CSRC) if os.path.basename(p) not in ("switches.hpp", "switches.hip") and "getenv" in _read(p)]
    assert not hits, "getenv outside switches.hip: %s" % hits


def test_section8_lists_the_table():
    table, (doc, _) = _table_names(), _section8()
    assert len(table) > 40   # (the regular expression still reads the list)
    assert table == doc, "only in switches.hpp: %s; only in DESIGN.md section 8: %s" % (sorted(table - doc), sorted(doc - table))


def test_section8_keeps_the_order_of_the_table():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    sec = text[text.index("\n## 8. Environment switches"):text.index("Not read by the library:")]
    assert re.findall(r"^\| `(EMAGLS_\w+)`", sec, re.M) == ["EMAGLS_" + n for n in re.findall(r"^\s*X\((\w+),", _read(os.path.join(CSRC, "switches.hpp")), re.M)]


def test_names_set_by_tests_and_tools_exist():
    table, (_, other) = _table_names(), _section8()
    api = set(re.findall(r"EMAGLS_\w+", _read(os.path.join(ROOT, "include", "emagls.h"))))   # constants of the C API are no switches
    used = {}
    tops = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    for top in tops:
        for p in _files(top, skip=(os.path.join(ROOT, "tools", "experiments"),)):
            if not p.endswith(".py") or os.path.abspath(p) == os.path.abspath(__file__):
                continue
            src = _read(p)
            names = re.findall(r"""(?:setenv|delenv|environ\.get|environ\.pop|environ\.setdefault)\(\s*["'](EMAGLS_\w+)["']""", src)
            names += re.findall(r"""environ\[\s*["'](EMAGLS_\w+)["']\s*\]""", src)
            for lit in re.findall(r"\benv\s*=\s*(?:dict\(\s*os\.environ\s*,\s*\*\*)?\{([^{}]*)\}", src):   # keys of an env= dictionary literal
                names += re.findall(r"""["'](EMAGLS_\w+)["']\s*:""", lit)
            for n in names:
                used.setdefault(n, os.path.relpath(p, ROOT))
    assert used   # (the patterns still find what the tests set)
    unknown = {n: p for n, p in used.items() if n not in table and n not in other and n not in api and not TEST_ONLY.match(n)}
    assert not unknown, "set or read, but neither in switches.hpp nor in DESIGN.md section 8: %s" % unknown


def test_retired_switches_stay_out():
    tops = [os.path.join(ROOT, d) for d in ("emagls_amd", "include", "mex", "tests", "tools")]
    hits = []
    for top in tops:
        for p in _files(top, skip=(os.path.join(ROOT, "tools", "experiments"), os.path.join(ROOT, "emagls_amd", "build"), os.path.join(ROOT, "emagls_amd", "lib"))):
            if os.path.abspath(p) == os.path.abspath(__file__) or p.endswith((".so", ".o", ".npy", ".npz", ".mat", ".h5", ".sofa", ".bin")):
                continue
            src = _read(p)
            hits += ["%s: %s" % (os.path.relpath(p, ROOT), n) for n in RETIRED if re.search(n + r"\b", src)]
    src = _read(os.path.join(ROOT, "bench.py"))
    hits += ["bench.py: %s" % n for n in RETIRED if re.search(n + r"\b", src)]
    assert not hits, hits
