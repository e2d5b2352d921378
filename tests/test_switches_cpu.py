"""The rule of INTEGRATION.md, "Environment switches": a compile-time macro or an environment switch of the native library exists only if a
test or a tool of this tree sets it or reads its effect, and it is documented.  Plain text processing of etude_amd/csrc:

  * every string literal passed to getenv( or ETD_XENV( appears in INTEGRATION.md's switch tables and in some .py / .sh under tests/ or tools/
    (the two fault-localising switches INTEGRATION.md keeps as its documented procedure are the exception to the second half);
  * every macro tested by #if / #ifdef / #ifndef / #elif appears in tools/README.md or INTEGRATION.md (the compiler's own macros and the two
    operand-type macros the headers derive from the documented -DETD_*_BF16 are exempt)."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "etude_amd" / "csrc"
DOCUMENTED_PROCEDURE = {"ETD_LAUNCH_LOG", "ETD_NO_GRAPH"}
EXEMPT_MACROS = {"__HIPCC__", "__HIP_DEVICE_COMPILE__", "ETD_DEC_IS_F16", "ETD_EXT_IS_F16"}


def _sources():
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".cpp", ".h"))
    assert len(files) > 40, "etude_amd/csrc not found where the test expects it"
    return [(p, p.read_text()) for p in files]


def _switch_tables():
    text = (ROOT / "INTEGRATION.md").read_text()
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    return "\n".join(ln for ln in section.split("\n") if ln.startswith("|"))


def _users():
    """text of every script under tests/ and tools/ (this file names the exceptions, so it does not count)"""
    out = []
    for d in ("tests", "tools"):
        for p in (ROOT / d).rglob("*"):
            if p.suffix in (".py", ".sh") and p.resolve() != Path(__file__).resolve():
                out.append(p.read_text(errors="replace"))
    return "\n".join(out)


def _word(name, text):
    """`name` as a whole word, or as the compiler option -Dname"""
    return re.search(r"(?:(?<![A-Za-z0-9_])|(?<=-D))" + re.escape(name) + r"(?![A-Za-z0-9_])", text) is not None


def test_every_environment_switch_is_documented_and_has_a_user():
    tables, users = _switch_tables(), _users()
    calls, names = 0, {}
    for p, src in _sources():
        for m in re.finditer(r"\b(?:getenv|ETD_XENV)\s*\(\s*([^)]*)\)", src):
            if p.name == "common.h" and m.group(1).strip() == "name":      # ETD_XENV's own definition
                continue
            calls += 1
            lit = re.fullmatch(r'"([^"]+)"', m.group(1).strip())
            assert lit, f"{p.name}: the environment is read through something that is no string literal: {m.group(0)}"
            names.setdefault(lit.group(1), p.name)
    assert calls >= 10 and "ETD_FUSED_PMLP" in names, "the scan found no switches: the pattern no longer matches the sources"
    undocumented = sorted(n for n in names if not _word(n, tables))
    assert not undocumented, f"switches missing from INTEGRATION.md's tables: {undocumented}"
    unused = sorted(n for n in names if n not in DOCUMENTED_PROCEDURE and not _word(n, users))
    assert not unused, f"switches that no test or tool sets (remove them, or add their user): {unused}"


def test_every_conditional_macro_is_documented():
    docs = (ROOT / "tools" / "README.md").read_text() + (ROOT / "INTEGRATION.md").read_text()
    seen = {}
    for p, src in _sources():
        for m in re.finditer(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b([^\n]*)", src, re.M):
            cond = re.sub(r"/\*.*?\*/|//.*", "", m.group(2))
            for name in re.findall(r"[A-Za-z_]\w*", cond):
                if name != "defined":
                    seen.setdefault(name, p.name)
    assert "ETD_EXPERIMENTS" in seen and "__HIPCC__" in seen, "the scan found no conditionals: the pattern no longer matches the sources"
    undocumented = sorted(f"{n} ({f})" for n, f in seen.items() if n not in EXEMPT_MACROS and not _word(n, docs))
    assert not undocumented, f"macros tested by the preprocessor that neither tools/README.md nor INTEGRATION.md names: {undocumented}"
