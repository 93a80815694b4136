"""The constants of include/mythgpu.h, read from the header itself.

The header is the one definition of the device interface's numbers; this module
parses it once at import and exposes, as module attributes,

- every integer ``#define MG_*`` (``DEFINES``): decimal or hex literals with
  ``u`` / ``ull`` suffixes, shifts, sums and other ``MG_*`` names;
- kernel 2's opcodes: ``BV_OPS``, the ``(C name, host name)`` pairs of
  ``MG_BV_OP_LIST`` in order, and the enumerators ``MG_BV_<C name>`` with
  ``MG_BV_NUM_OPS`` (``BV_ENUM``).

A definition the parser cannot evaluate raises at import: no name is skipped.
"""
from __future__ import annotations

import re
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "mythgpu.h"

_DEFINE = re.compile(r"^#define[ \t]+(MG_\w+)[ \t]+(.*)$", re.M)     # object-like macros only
_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?[lL]{0,2})\b|(MG_\w+)|(<<|>>|[-+*|&~()]))")
_OP_LIST = re.compile(r"^#define[ \t]+MG_BV_OP_LIST\(X\)((?:.*\\\n)*.*)$", re.M)
_OP = re.compile(r'X\((\w+),\s*"([^"]+)"\)')


def _evaluate(name: str, text: str, known: dict) -> int:
    text = text.split("/*")[0].strip()
    out, pos = [], 0
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m or (m.group(2) and m.group(2) not in known):
            raise ImportError(f"{HEADER}: cannot evaluate #define {name} {text!r}")
        out.append(m.group(1) or m.group(3) or str(known[m.group(2)]))
        pos = m.end()
    try:
        return int(eval(" ".join(out), {"__builtins__": {}}))    # integers and operators only
    except Exception as e:
        raise ImportError(f"{HEADER}: cannot evaluate #define {name} {text!r}: {e}") from None


def parse(source: str):
    defines: dict = {}
    for name, text in _DEFINE.findall(source):
        defines[name] = _evaluate(name, text, defines)
    ops = _OP_LIST.search(source)
    if not ops or not _OP.search(ops.group(1)):
        raise ImportError(f"{HEADER}: no MG_BV_OP_LIST")
    return defines, [(c, host) for c, host in _OP.findall(ops.group(1))]


DEFINES, BV_OPS = parse(HEADER.read_text())
BV_ENUM = {f"MG_BV_{c}": i for i, (c, _) in enumerate(BV_OPS)}
BV_ENUM["MG_BV_NUM_OPS"] = len(BV_OPS)
globals().update(DEFINES)
globals().update(BV_ENUM)
__all__ = [*DEFINES, *BV_ENUM]
