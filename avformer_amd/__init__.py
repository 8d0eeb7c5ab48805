"""Importable alias of the package directory
``multi-modal-multi-label-facial-action-unit-detection-with-transformer_amd`` (its name is not a
Python identifier, so ``import avformer_amd`` is the convenient spelling)."""
import importlib
import os
import sys

_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _root not in sys.path:
    sys.path.insert(0, _root)
PACKAGE = "multi-modal-multi-label-facial-action-unit-detection-with-transformer_amd"
_pkg = importlib.import_module(PACKAGE)
sys.modules[__name__] = _pkg
# ... and its submodules under the alias too: `from avformer_amd.transformer import x` must find the module that is loaded, not
# import a second copy of it (and, through its relative imports, of _lib: two sets of ctypes structures that refuse each other)
for _name, _mod in list(sys.modules.items()):
    if _name.startswith(PACKAGE + "."):
        sys.modules[__name__ + _name[len(PACKAGE):]] = _mod
