"""What the call-dump probes (float_conv_call_dump.py, int8_conv_call_dump.py) share: the proxy that records every call made
through _native.lib(), and the naming of a recorded pointer by the operand it points into."""
import ctypes


class Recorder(object):
    """Stands in for the ctypes library: every function called through it is noted as (name, args) and forwarded."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def show_arg(a, named):
    """One recorded argument as text: `null`, `stream`, `<operand name>+<byte offset>` for a pointer into one of the
    (name, tensor) pairs of `named` -- the first that holds it, so the order of `named` decides, not the addresses -- and the
    repr of anything else (the integers and floats of the ABI)."""
    if a is None:
        return "null"
    if isinstance(a, ctypes.c_void_p):
        return "stream"
    if isinstance(a, int):
        for name, t in named:
            off = a - t.data_ptr()
            if 0 <= off < max(t.numel() * t.element_size(), 1):
                return "%s+%d" % (name, off)
    return repr(a)
