"""What the Python restatements of the kernels' rules (tests/tiled_model.py, tests/fused_model.py) share for reading
constants out of the sources: a C integer constant expression evaluated as Python does, a regular expression that must match."""
import re


def c_int(expr, names):
    """A C constant expression of unsigned integers (+ - * / parentheses, names defined before) as Python computes it."""
    e = re.sub(r"\b(\d+)[uU]?[lL]{0,2}\b", r"\1", expr.strip())
    if not re.fullmatch(r"[\w\s+\-*/()]+", e):
        raise ValueError("not an integer constant expression: %r" % expr)
    return int(eval(e.replace("/", "//"), {"__builtins__": {}}, dict(names)))


def one(pattern, text, what, who="tests/tiled_model.py"):
    m = re.search(pattern, text)
    if not m:
        raise AssertionError("%s no longer finds %s in the sources" % (who, what))
    return m
