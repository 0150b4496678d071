"""What the feature maps RFFMap (rff.py) and NystroemMap (nystroem.py) share: the handle's life, the samples a call reads and the output it makes."""
import ctypes as ct

import numpy as np

from ._lib import check
from .core import DeviceSamples
from .mat import is_sparse

TYPE_CODES = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # PMH_F64, PMH_F32


class FeatureMap:
    """A subclass sets ENTRY (the prefix of its C entries) and INFO (the names of pmh_<entry>_info's 8 integers), and on an instance ctx, L (the library), h (the
    handle, None once destroyed) and d (the width of the samples it reads).  Its own name leads the messages."""
    ENTRY = INFO = None

    def _need(self):
        if self.h is None:
            raise RuntimeError("%s: the map has been destroyed" % type(self).__name__)

    def info(self):
        """What pmh_<entry>_info reports, as a dict over the class's INFO: the tiling of the kernels, then the two sizes that are the class's own."""
        self._need()
        v = (ct.c_int * 8)()
        check(getattr(self.L, self.ENTRY + "_info")(self.h, v))
        return dict(zip(self.INFO, (int(x) for x in v)))

    def _out_dtype(self, out_dtype):
        odt = np.dtype(out_dtype)
        if odt not in TYPE_CODES:
            raise ValueError("%s.transform: out_dtype must be numpy.float64 or numpy.float32, not %r" % (type(self).__name__, out_dtype))
        return odt

    def _source(self, X):
        """X as (DeviceSamples, made here): an ndarray goes up as float32 if it is float32 and as float64 otherwise."""
        name = type(self).__name__
        if is_sparse(X):
            raise TypeError("%s.transform: X is a scipy.sparse matrix; sparse samples are not supported by the map (it reads dense rows): pass X.toarray(), or dense blocks of rows" % name)
        if isinstance(X, DeviceSamples):
            src, made = X, False
        else:
            src, made = DeviceSamples.from_numpy(self.ctx, X), True
        if src.d != self.d:
            if made:
                src.free()
            raise ValueError("%s: X must be (n, %d), not (n, %d)" % (name, self.d, src.d))
        return src, made

    def _run(self, X, width, dtype, call):
        """call(src, out) on X as the device sees it and a new DeviceSamples (n, self.<width>) of dtype, which is returned."""
        src, made = self._source(X)
        out = None
        try:
            self._need()
            out = DeviceSamples.empty(self.ctx, src.n, getattr(self, width), dtype)
            check(call(src, out))
            res, out = out, None
            return res
        finally:
            if out is not None:
                out.free()
            if made:
                src.free()

    def _run_host(self, X, width, call):
        """_run for the tests' entries: the (n, self.<width>) float64 result as a host array."""
        T = self._run(X, width, np.float64, call)
        try:
            return T.numpy()
        finally:
            T.free()

    def destroy(self):
        if self.h is not None:
            getattr(self.L, self.ENTRY + "_destroy")(self.h)
            self.h = None
