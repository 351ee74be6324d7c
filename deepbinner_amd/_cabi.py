"""The one way this package binds a C ABI with ctypes (``hip_backend``, ``fast5_native``,
``dtw_semi_global``): a table ``{name: (restype, argtypes)}`` typed onto a loaded library, and a
base for the Python objects that own one handle of such a library.  Where the library lies, what
to say when it is not built, and the load-once cache stay with each binding module."""

import ctypes


def bind(path, signatures):
    """Load the shared library at ``path`` and give every function of ``signatures`` its
    ``restype`` and ``argtypes``; returns the ctypes handle.  Raises OSError where the library does
    not load, AttributeError where it lacks one of the table's symbols."""
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AttributeError('{} does not export {}: header and library are out of step'
                                 .format(path, name)) from None
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


class Owner:
    """An object that holds one handle of a C library.  A subclass keeps the library in
    ``self._lib`` and names, as class attributes, the attribute that holds the handle (``_held``)
    and the library's function that gives it back (``_release``); ``close()`` releases it once.
    ``with`` and a finaliser are not part of it: a class opts in with Scoped and Finalised."""

    _held, _release = '_handle', None

    def close(self):
        handle = getattr(self, self._held, None)    # (None too where __init__ did not get that far)
        if handle:
            getattr(self._lib, self._release)(handle)
            setattr(self, self._held, None)


class Scoped:
    """``with owner:`` closes it on the way out."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Finalised:
    """The garbage collector closes what nobody closed."""

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
