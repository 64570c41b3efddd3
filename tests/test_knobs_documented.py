"""INTEGRATION.md §5 lists exactly the DD_* environment variables the library and the package
read, and the library reads them only through the helpers of csrc/dd_common.h."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "data_diet_distributed_amd", "csrc")
PKG = os.path.join(ROOT, "data_diet_distributed_amd")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _csrc_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def _library_knobs():
    names = set()
    for path in _csrc_files():
        names |= set(re.findall(r'\benv_(?:int|str)\(\s*"(\w+)"', _read(path)))
    return names


def _package_vars():
    names = set()
    for path in glob.glob(os.path.join(PKG, "*.py")):
        names |= set(re.findall(r'os\.environ(?:\.get\(|\.setdefault\(|\[)\s*"(DD_\w+)"',
                                _read(path)))
        names |= set(re.findall(r'"(DD_\w+)"\s+in\s+os\.environ', _read(path)))
    return names


def _documented():
    """Names in the first column of the tables of INTEGRATION.md §5 (to the end of the file or
    the next top-level section)."""
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    sec = text[text.index("\n## 5. "):]
    nxt = sec.find("\n## ", 1)
    if nxt > 0:
        sec = sec[:nxt]
    return set(re.findall(r"^\| `(DD_\w+)` \|", sec, flags=re.M))


def test_every_variable_read_is_in_the_table_and_nothing_else():
    lib, pkg = _library_knobs(), _package_vars()
    assert lib and pkg, "the collectors found nothing: the patterns no longer match the code"
    assert all(n.startswith("DD_") for n in lib), sorted(lib)
    assert lib | pkg == _documented()


def test_no_bare_getenv_in_the_library():
    bare = [os.path.basename(p) for p in _csrc_files()
            if os.path.basename(p) != "dd_common.h" and "getenv(" in _read(p)]
    assert bare == []
