"""A SEA_TUNE key that a test forces must be read by the library on EVERY call.  A key held in a function-local `static` is fixed by the first call of
the process: in a whole-suite run it is read unset long before the forcing test starts, and that test then runs the default form and passes.  This lint
keeps the keys the tests put into SEA_TUNE and the keys sea_amd/csrc/*.hip reads through a static initialiser apart."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CSRC = os.path.join(ROOT, "sea_amd", "csrc")

_READ = re.compile(r'sea_tune\(\s*"([A-Za-z0-9_]+)"')
_STATIC_READ = re.compile(r'\bstatic\b[^;]*?sea_tune\(\s*"([A-Za-z0-9_]+)"')
# the two spellings the suite uses: setenv("SEA_TUNE", "...") and {"SEA_TUNE": "..."} (plain or f-strings)
_SETENV = re.compile(r'setenv\(\s*["\']SEA_TUNE["\']\s*,\s*[fFrR]*(["\'])(.*?)\1')
_DICT = re.compile(r'["\']SEA_TUNE["\']\s*:\s*[fFrR]*(["\'])(.*?)\1')
_LITERAL = re.compile(r'[fFrR]*(["\'])((?:[A-Za-z0-9_]+=[^,"\']*)(?:,[A-Za-z0-9_]+=[^,"\']*)*)\1')
_KEY = re.compile(r'(?:^|,)\s*([A-Za-z0-9_]+)=')


def library_keys(csrc=CSRC):
    """{key: [(file name, line number, static?)]} of every sea_tune("key", ...) read in the .hip sources."""
    out = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        with open(path) as f:
            for no, line in enumerate(f, 1):
                static = set(_STATIC_READ.findall(line))
                for key in _READ.findall(line):
                    out.setdefault(key, []).append((os.path.basename(path), no, key in static))
    return out


def forced_keys(tests=TESTS, known=()):
    """{key: [(test file, line number)]}: keys of both SEA_TUNE spellings, and — for values that reach setenv through a variable or a helper — of every string
    literal made only of key=value tokens whose keys are all ones the library reads (`known`), in a file that names SEA_TUNE."""
    out = {}
    for path in sorted(glob.glob(os.path.join(tests, "**", "*.py"), recursive=True)):
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        with open(path) as f:
            lines = f.readlines()
        if not any("SEA_TUNE" in l for l in lines):
            continue
        for no, line in enumerate(lines, 1):
            values = [m.group(2) for rx in (_SETENV, _DICT) for m in rx.finditer(line)]
            for m in _LITERAL.finditer(line):
                keys = _KEY.findall(m.group(2))
                if keys and all(k in known for k in keys):
                    values.append(m.group(2))
            for v in values:
                for key in _KEY.findall(v):
                    if (os.path.basename(path), no) not in out.setdefault(key, []):
                        out[key].append((os.path.basename(path), no))
    return out


def clashes(csrc=CSRC, tests=TESTS):
    lib = library_keys(csrc)
    forced = forced_keys(tests, known=set(lib))
    msgs = []
    for key in sorted(set(forced) & {k for k, reads in lib.items() if any(s for _, _, s in reads)}):
        for src, no, static in lib[key]:
            if static:
                for tfile, tno in forced[key]:
                    msgs.append(f"SEA_TUNE key '{key}' is forced by tests/{tfile}:{tno} but read once per process (static) at sea_amd/csrc/{src}:{no}")
    return msgs


def test_the_suite_forces_something_and_the_library_reads_it():
    """The collectors see what is there: both spellings, f-strings, and every key a test forces is one the library reads at all."""
    lib = library_keys()
    forced = forced_keys(known=set(lib))
    for key in ("gemm256", "gemm_ws", "attn_paired", "attnb_mode", "chain_rows", "kv_persist", "sse_rows", "gemm_norm_rows"):
        assert key in forced, key            # gemm_norm_rows: the dict spelling (test_model_gpu.py); attnb_mode / chain_rows: f-strings
    assert any(f == "test_model_gpu.py" for f, _ in forced["gemm_norm_rows"])
    assert len(lib) >= 30
    for key, where in forced.items():
        assert key in lib, f"SEA_TUNE key '{key}' (tests/{where[0][0]}:{where[0][1]}) is read nowhere in sea_amd/csrc"


def test_no_forced_key_is_read_through_a_static():
    msgs = clashes()
    assert not msgs, "\n".join(msgs)


def test_lint_reports_a_restored_static(tmp_path):
    """The lint against itself: a copy of one source line with `static` put back must be reported, with the key, the test file and the source line."""
    src = os.path.join(CSRC, "gemm_norm.hip")
    with open(src) as f:
        lines = f.readlines()
    hits = [i for i, l in enumerate(lines) if 'sea_tune("gemm_norm_rows"' in l]
    assert len(hits) == 1 and "static" not in lines[hits[0]]
    assert re.search(r"^\s*const int forced", lines[hits[0]])
    (tmp_path / "gemm_norm.hip").write_text("\n" * hits[0] + lines[hits[0]].replace("const int forced", "static const int forced", 1))
    msgs = clashes(csrc=str(tmp_path))
    assert msgs and all("'gemm_norm_rows'" in m and f"gemm_norm.hip:{hits[0] + 1}" in m for m in msgs)
    assert any("tests/test_model_gpu.py:" in m for m in msgs)
    (tmp_path / "gemm_norm.hip").write_text("\n" * hits[0] + lines[hits[0]])   # ... and the line as it is, is clean
    assert clashes(csrc=str(tmp_path)) == []
