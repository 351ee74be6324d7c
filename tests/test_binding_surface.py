"""The bindings' shape: hip_backend's facade exports what the one-file module did and defines
nothing itself, each binding module keeps its C ABI in one table, and _cabi names a symbol the
library lacks.  No GPU."""
import ast
import ctypes
import importlib
import os
import pkgutil
import types

import pytest

from conftest import REPO
from deepbinner_amd import _cabi, dtw_semi_global, fast5_native, hip_backend

PACKAGE_DIR = os.path.dirname(hip_backend.__file__)
SUBMODULES = [importlib.import_module(hip_backend.__name__ + '.' + info.name)
              for info in pkgutil.iter_modules([PACKAGE_DIR])]


def test_facade_exports_the_names_of_the_one_file_module():
    with open(os.path.join(REPO, 'tests', 'golden', 'hip_backend_names.txt')) as f:
        names = f.read().split()
    assert len(names) == 90          # (the 88 of the one-file module, fill_lds and survey_lds)
    missing = [name for name in names if not hasattr(hip_backend, name)]
    assert not missing, missing
    from deepbinner_amd.hip_backend import _TensorSpec       # what tests/conftest.py imports
    assert _TensorSpec is hip_backend._model._TensorSpec


def test_facade_defines_nothing_of_its_own():
    assert len(SUBMODULES) >= 8
    for name, value in vars(hip_backend).items():
        if name.startswith('_') or isinstance(value, types.ModuleType):
            continue
        assert any(vars(module).get(name, hip_backend) is value for module in SUBMODULES), name
    tree = ast.parse(open(hip_backend.__file__).read())
    assert all(isinstance(node, ast.ImportFrom) or
               (isinstance(node, ast.Expr) and isinstance(node.value, ast.Constant))
               for node in tree.body)


def test_submodules_are_layered_and_leave_the_facade_alone():
    """No submodule imports the facade, and none imports a submodule that imports it back: each
    builds only on those before it, with the ABI module under all."""
    imports = {}
    for module in SUBMODULES:
        short = module.__name__.rsplit('.', 1)[1]
        wanted = set()
        for node in ast.walk(ast.parse(open(module.__file__).read())):
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                assert node.module, '{} imports the facade'.format(short)
                wanted.add(node.module)
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                assert 'hip_backend' not in ast.dump(node), short
        imports[short] = wanted
        assert len(open(module.__file__).readlines()) <= 460, short
    assert imports['_abi'] == set()
    placed = []
    while len(placed) < len(imports):
        ready = [m for m in imports if m not in placed and imports[m] <= set(placed)]
        assert ready, 'a cycle among {}'.format(sorted(set(imports) - set(placed)))
        placed += ready
    assert placed[0] == '_abi' and all(imports[name] for name in placed[1:])


@pytest.mark.parametrize('module', [hip_backend, fast5_native, dtw_semi_global],
                         ids=lambda module: module.__name__.rsplit('.', 1)[1])
def test_one_table_per_library(module):
    assert module.EXPORTED_SYMBOLS == list(module.SIGNATURES)
    lib = module.load_library()
    for name, (restype, argtypes) in module.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert module.load_library() is lib


def test_state_lives_in_one_submodule():
    for name in ('_lib', '_PINNED_LOADER'):
        assert [m.__name__ for m in SUBMODULES if name in vars(m)] == \
            [hip_backend.__name__ + {'_lib': '._abi', '_PINNED_LOADER': '._device'}[name]]
        assert name not in vars(hip_backend)


def test_cabi_names_the_symbol_a_library_lacks():
    path = fast5_native.library_path()
    table = {'f5_version': (ctypes.c_char_p, []), 'f5_no_such_function': (ctypes.c_int, [])}
    with pytest.raises(AttributeError) as e:
        _cabi.bind(path, table)
    assert 'f5_no_such_function' in str(e.value) and 'out of step' in str(e.value)
    lib = _cabi.bind(path, {'f5_version': table['f5_version']})
    assert isinstance(lib.f5_version(), bytes)


def test_owner_lifetimes_are_the_classes_own():
    """close() on every owner; ``with`` and a finaliser only where the class had them."""
    from deepbinner_amd._cabi import Finalised, Owner, Scoped
    want = {hip_backend.DeviceBuffer: (False, True), hip_backend.Event: (False, True),
            hip_backend.Stream: (False, False), hip_backend.HipModel: (False, True),
            hip_backend.Dataset: (True, True), hip_backend.Trainer: (True, True),
            hip_backend.ResidentText: (True, False), fast5_native.File: (True, True)}
    for cls, (scoped, finalised) in want.items():
        assert issubclass(cls, Owner) and callable(cls.close), cls
        assert issubclass(cls, Scoped) == scoped == hasattr(cls, '__enter__'), cls
        assert issubclass(cls, Finalised) == finalised == hasattr(cls, '__del__'), cls
    assert hip_backend.DeviceBuffer.free is Owner.close

    released = []

    class Lib:
        @staticmethod
        def give_back(handle):
            released.append(handle)

    class Thing(Owner, Scoped, Finalised):
        _held, _release = 'ptr', 'give_back'

        def __init__(self, ptr):
            self._lib, self.ptr = Lib, ptr

    with Thing(7) as thing:
        assert thing.ptr == 7
    thing.close()
    assert released == [7] and thing.ptr is None
    Thing(9).__del__()
    Thing(None).close()
    assert released == [7, 9]
    broken = Thing.__new__(Thing)            # __init__ never ran: the finaliser has nothing to do
    broken.__del__()
    assert released == [7, 9]
