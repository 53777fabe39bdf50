"""The switch table of docs/NOTES.md ("Environment switches") lists exactly the literal
MPA_* names that the package, csrc/, bench.py and setup.py read from the environment."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_READ = re.compile(r'(?:environ(?:\.get)?\s*[\[(]\s*|getenv\s*\(\s*|\benv\.get\(\s*)"(MPA_[A-Z0-9_]+)"'
                   r'|"(MPA_[A-Z0-9_]+)"\s+in\s+os\.environ')


def _sources():
    files = [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "setup.py")]
    for top, exts in (("mpi_pytorch_amd", (".py",)), ("csrc", (".hip", ".h", ".cpp", ".hpp"))):
        for ext in exts:
            files += glob.glob(os.path.join(ROOT, top, "**", "*" + ext), recursive=True)
    return files


def test_switch_table_matches_sources():
    read = set()
    for f in _sources():
        with open(f) as fh:
            for m in _READ.finditer(fh.read()):
                read.add(m.group(1) or m.group(2))
    with open(os.path.join(ROOT, "docs", "NOTES.md")) as fh:
        text = fh.read()
    table = text[text.index("## Environment switches"):]
    listed = re.findall(r"^\| `(MPA_[A-Z0-9_]+)` \|", table, re.M)
    assert len(listed) == len(set(listed)), "a switch is listed twice"
    assert len(read) > 40  # (the collector still finds the reads)
    assert set(listed) == read, (sorted(read - set(listed)), sorted(set(listed) - read))
