#!/usr/bin/env python3
"""Print the Python surface of the native module, one sorted record per public name.

For the module and each of its submodules: the kind of every name, the docstring of every function
(pybind11's signature line carries argument names, types and defaults), every attribute of every
class with its docstring (a property's getter docstring too) and the value of every plain value.
Two builds bind the same surface exactly when their outputs are equal:

    python tools/native_surface.py > surface.txt
"""
from __future__ import annotations

import importlib
import sys
import types
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def doc(o) -> str:
    return repr(getattr(o, "__doc__", None))


def records(mod: types.ModuleType, prefix: str):
    for name, o in vars(mod).items():
        if name.startswith("_"):
            continue
        q = f"{prefix}.{name}"
        if isinstance(o, types.ModuleType):
            yield f"{q} module {doc(o)}"
            yield from records(o, q)
        elif isinstance(o, type):
            bases = ",".join(b.__name__ for b in o.__bases__)
            yield f"{q} class({bases}) is={o.__module__}.{o.__qualname__} {doc(o)}"
            for attr, v in vars(o).items():
                if attr in ("__module__", "__dict__", "__weakref__"):
                    continue
                line = f"{q}.{attr} {type(v).__name__} {doc(v)}"
                if isinstance(v, property):
                    line += f" fget={doc(v.fget)} fset={doc(v.fset) if v.fset else None}"
                yield line
        elif callable(o):
            yield f"{q} function {doc(o)}"
        else:
            yield f"{q} value {type(o).__name__} {o!r}"


def main() -> None:
    mod = importlib.import_module("video_edge_ai_proxy_amd._vep")
    print(f"_vep module {doc(mod)}")
    for line in sorted(records(mod, "_vep")):
        print(line)


if __name__ == "__main__":
    main()
