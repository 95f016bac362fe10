"""One work area per consulted launch, registered in one place: of all the code of the Tacotron models only one function
assigns into _status_words, so no launch site can register a work area that another launch of the step clears.

The three model files are parsed, not imported (as in test_graph_sections_cpu.py).
"""
import ast
import os

MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nspeech_amd", "models")
FILES = ("tacotron2.py", "tacotron2_infer.py", "tacotron.py")


def _is_status_words(node):
    return (isinstance(node, ast.Subscript) and isinstance(node.value, ast.Attribute) and node.value.attr == "_status_words")


def _assigning_functions():
    """(file, function) of every function whose own body assigns to a subscript of <anything>._status_words."""
    found = []
    for name in FILES:
        with open(os.path.join(MODELS, name)) as f:
            tree = ast.parse(f.read(), name)
        for fn in ast.walk(tree):
            if not isinstance(fn, (ast.FunctionDef, ast.Lambda)):
                continue
            for node in ast.walk(fn):
                targets = []
                if isinstance(node, ast.Assign):
                    targets = node.targets
                elif isinstance(node, (ast.AugAssign, ast.AnnAssign)):
                    targets = [node.target]
                flat = [e for t in targets for e in (t.elts if isinstance(t, (ast.Tuple, ast.List)) else [t])]
                if any(_is_status_words(t) for t in flat):
                    found.append((name, getattr(fn, "name", "<lambda>")))
    return found


def test_one_function_registers_status_words():
    found = _assigning_functions()
    # an enclosing function would be listed beside a nested one: the helper is a plain method, so exactly one entry
    assert found == [("tacotron2.py", "_persistent")], found


def test_adam_takes_32_status_words():
    """Version 108: ns_adam_params.status has NS_ADAM_STATUS_MAX = 32 entries, and the binding sizes its array from the
    same constant of the header."""
    from nspeech_amd import _lib
    assert _lib.NS_ADAM_STATUS_MAX == 32 and len(_lib.struct("ns_adam_params").status) == 32
    assert _lib.lib().ns_version() >= 108


def test_no_other_way_in():
    """No setdefault / update / __setitem__ call on _status_words either."""
    calls = []
    for name in FILES:
        with open(os.path.join(MODELS, name)) as f:
            tree = ast.parse(f.read(), name)
        for node in ast.walk(tree):
            if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)
                    and node.func.attr in ("setdefault", "update", "__setitem__")
                    and isinstance(node.func.value, ast.Attribute) and node.func.value.attr == "_status_words"):
                calls.append((name, node.lineno))
    assert not calls, calls
