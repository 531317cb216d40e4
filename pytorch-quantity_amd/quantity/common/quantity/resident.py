"""Resident integer activations for the integer-simulation model (ReconModel).

The reference's NewConv2d / NewAdd hand fp32 NCHW tensors from module to module
(new_quantity_op.py:124-133, :171-174): DeQuantity writes 4 bytes per activation, nn.ReLU reads and
writes them, the next layer's Quantity reads them again and recovers -- exactly -- the integer the
previous layer's tail already held.  `enable(model, example)` keeps that integer in HBM instead:

  * one traced forward (module hooks + a TorchFunctionMode) records, for the output of every
    NewConv2d / NewAdd, who consumes it: another integer layer, a ReLU, or anything else;
  * producers whose consumers are integer layers emit int8 NHWC straight from the MFMA epilogue
    (conv) or int16 + int8 NHWC from the fused add kernel, with the following nn.ReLU folded in
    (max(., 0) commutes with the power-of-two scale); consumers read those bytes directly;
  * anything else still receives the ordinary fp32 NCHW tensor (a value used by both kinds gets both).

Every resident value is `integer * 2^-grid` and stands for exactly the fp32 number the reference
would have produced, so model outputs are bit-identical to the fp32-boundary path
(tests/test_gpu_resident.py); the saving is HBM traffic: 18-29 bytes per activation become 2-6.

The plan assumes a static dataflow (as a captured graph would).  Consumers stay adaptive -- a layer
that unexpectedly receives fp32 quantises it as usual -- and a resident handle reaching code that
is not part of the plan raises instead of computing garbage.
"""
import collections
import os

import torch
from torch import nn
from torch.overrides import TorchFunctionMode

from . import _native

__all__ = ["QHandle", "enable", "disable", "is_enabled", "describe", "capture", "GraphedForward", "MultiStreamGraphs"]

MAX_WIDE_GRID = 8          # int16 holds |s| <= 128 on a grid of 2^-8


class QHandle(object):
    """An activation kept as integers in HBM.  Not a tensor on purpose: code outside the plan that
    touches it fails loudly.

    exact : int8 / int16 NHWC tensor, value = exact * 2^-grid (the reference's fp32 value, exactly)
    narrow: int8 NHWC tensor = Quantity(value, bit) for the next conv (conv outputs: the same tensor)
    """
    __slots__ = ("shape", "exact", "grid", "narrow", "bit", "relu_done", "next_out", "lossy")

    def __init__(self, shape, exact, grid, narrow, bit, relu_done):
        self.shape, self.exact, self.grid, self.narrow, self.bit, self.relu_done = shape, exact, grid, narrow, bit, relu_done
        # (consumer NewConv2d, its finished output handle): set by a NewAdd that ran that consumer inside its own kernel
        # (fq_block_tail_i8, Plan.fuse_next) -- the consumer hands it out instead of launching
        self.next_out = None
        # made by the table kernel (enable(activations=True)), or moved from such a handle: the integers are Quantity_bit(f(x)),
        # not f(x) -- right for a convolution at that bit and for nothing else (to_f32 raises)
        self.lossy = False

    @classmethod
    def int8(cls, q, channels, bit, relu_done):
        """An int8 NHWC activation q = value * 2^bit: exact, and already what a convolution at that bit reads."""
        return cls((q.shape[0], channels, q.shape[1], q.shape[2]), q, bit, q, bit, relu_done)

    @classmethod
    def wide_narrow(cls, channels, wide, grid, narrow, bit, relu_done):
        """A sum: its exact integers on `grid` and / or its re-quantisation at `bit` (NHWC, at least one of the two)."""
        ref = wide if wide is not None else narrow
        return cls((ref.shape[0], channels, ref.shape[1], ref.shape[2]), wide, grid, narrow, bit, relu_done)

    def to_f32(self):
        """The fp32 NCHW tensor this handle stands for (DeQuantity + layout change, one kernel)."""
        if self.exact is None:
            raise _native.FqError("resident activation without an exact payload cannot leave the integer domain")
        if self.lossy:
            raise _native.FqError("the integers of a table activation are already quantised for the convolutions behind it and "
                                  "stand for no fp32 value (dataflow changed since resident.enable(); call it again)")
        return _native.dequant_nhwc_to_nchw(self.exact, self.grid, self.shape[1])

    def __repr__(self):
        return "QHandle(shape=%s, exact=%s@%s, narrow_bit=%s, relu=%s)" % (
            tuple(self.shape), None if self.exact is None else str(self.exact.dtype).replace("torch.", ""), self.grid,
            self.bit if self.narrow is not None else None, self.relu_done)


class DeferredConv(object):
    """A convolution whose only consumer is a resident NewAdd: nothing has been launched yet, the add runs
    it with the residual fused into its store phase (fq_conv2d_i8_add_resident), so the convolution's own
    int8 result never reaches HBM.  Anything else that touches it materialises the plain result."""
    __slots__ = ("layer", "xq", "wq", "geom", "_handle")

    def __init__(self, layer, xq, wq, geom):
        self.layer, self.xq, self.wq, self.geom, self._handle = layer, xq, wq, geom, None

    def materialise(self):
        if self._handle is None:
            L = self.layer
            _, q = _native.conv2d_i8_resident(self.xq, self.wq, L.quantized_bias, self.geom[0], self.geom[1], self.geom[2],
                                              L._rs(), L.output_bit, False, True, False)
            self._handle = QHandle.int8(q, L.Conv.out_channels, L.output_bit, False)
        return self._handle

    def to_f32(self):
        return self.materialise().to_f32()

    def pointwise(self, any_stride=False):
        return _pointwise(self.wq.shape[1:3], self.geom[0], self.geom[1], any_stride) and _pair(self.geom[2]) == (1, 1)


class DeferredUpsample(object):
    """A nearest upsampling whose only consumer is a resident Concat (enable(concat=True)): nothing has been launched, the
    Concat reads the small tensor with the factor as its operand's `up` (fq_concat_i8_nhwc), so the s*s times larger tensor is
    neither written nor read back.  Anything else that touches it materialises the upsampled activation.
    With enable(concat=True, topdown=True) the consumers are resident NewAdds (fq_add_up_resident) and the coarse handle's exact
    payload may be the int16 sum of another add.  No integer kernel upsamples int16: materialise() then returns the fp32 tensor
    that `module`'s own forward makes of the de-quantised coarse tensor (the values the reference computes), and resident_of()
    reports no integer form."""
    __slots__ = ("handle", "s", "_out", "module")

    def __init__(self, handle, s, module=None):
        self.handle, self.s, self._out, self.module = handle, int(s), None, module

    def materialise(self):
        if self._out is None:
            h = self.handle
            if h.exact is not None and h.exact.dtype == torch.int16:
                self._out = type(self.module).forward(self.module, h.to_f32())
                if h.relu_done:
                    self._out._fq_relu_done = True
            else:
                y = _native.concat_i8_nhwc([(h.exact, h.shape[1], self.s)], False)
                self._out = _moved(QHandle.int8(y, h.shape[1], h.grid, h.relu_done), h)
        return self._out

    def to_f32(self):
        out = self.materialise()
        return out.to_f32() if type(out) is QHandle else out


MAX_CONCAT_LEAVES = _native.CONCAT_N_MAX_SRC       # sources of one fq_concat_n_i8_nhwc launch


def _concat_launch(leaves):
    """One launch for the leaves [(handle, up, relu), ...] of a (flattened) Concat: the two-source function where it can say the
    same -- at most two leaves whose ReLU flags agree --, the N-source function otherwise."""
    flags = set(bool(r) for _h, _up, r in leaves)
    if len(leaves) <= 2 and len(flags) == 1:
        return _native.concat_i8_nhwc([(h.exact, h.shape[1], up) for h, up, _r in leaves], flags.pop())
    return _native.concat_n_i8_nhwc([(h.exact, h.shape[1], up, bool(r)) for h, up, r in leaves])


class DeferredConcat(object):
    """A resident Concat whose only consumer is another resident Concat (enable(concat=True, flatten=True)): nothing has been
    launched, the consumer takes these leaves -- (handle, upsampling factor, ReLU flag), the flag being this Concat's own fused
    nn.ReLU -- into its own source list and launches once (fq_concat_n_i8_nhwc), so the intermediate tensor is neither written
    nor read back.  Anything else that touches it materialises the concatenated activation."""
    __slots__ = ("leaves", "grid", "_out")

    def __init__(self, leaves, grid):
        self.leaves, self.grid, self._out = list(leaves), grid, None

    @property
    def relu_done(self):
        return all(r or h.relu_done for h, _up, r in self.leaves)

    def materialise(self):
        if self._out is None:
            q = _concat_launch(self.leaves)
            self._out = _moved(QHandle.int8(q, sum(h.shape[1] for h, _up, _r in self.leaves), self.grid, self.relu_done),
                               *[h for h, _up, _r in self.leaves])
        return self._out

    def to_f32(self):
        return self.materialise().to_f32()


def _moved(out, *sources):
    """`out`, a handle made by pure data movement or a max-pool of `sources`: it is lossy where one of them is."""
    out.lossy = any(h.lossy for h in sources)
    return out


def _moved_handle(h, y, channels):
    """The handle of y, the int8 integers of `h` moved or max-pooled into `channels` channels: on the source's grid, lossy where
    the source is, the narrow form carried where it equals the exact one."""
    narrow = y if (h.narrow is h.exact or h.bit == h.grid) else None
    return _moved(QHandle.wide_narrow(channels, y, h.grid, narrow, h.grid, h.relu_done), h)


def _lossy_int8(q, channels, bit, relu_done):
    """The handle of q = Quantity_bit(f(...)), the output of a kernel that re-quantises for the convolutions behind it: lossy."""
    out = QHandle.int8(q, channels, bit, relu_done)
    out.lossy = True
    return out


def block_tail_enabled():
    """FQ_BLOCK_TAIL=0: keep conv3 + add and the next conv1 as two launches (A/B timing).  Read at every call."""
    return os.environ.get("FQ_BLOCK_TAIL", "1") != "0"


def block_tail_proj_enabled():
    """FQ_BLOCK_TAIL_PROJ=0: a stage's first block keeps its projection shortcut as a launch of its own (A/B timing)."""
    return os.environ.get("FQ_BLOCK_TAIL_PROJ", "1") != "0"


def carry(t, handle):
    """Attach the integer form `handle` to the fp32 tensor t that stands for the same values (a producer that serves both kinds of
    consumers).  The attachment holds for the tensor AS WRITTEN BY ITS PRODUCER: its version counter is remembered, and a tensor
    that was written to since -- an in-place nn.ReLU between two consumers is legal PyTorch -- no longer has an integer form
    (resident_of).  Found by scripts/recon_fuzz.py: the consumer behind such a ReLU read the integers from before it."""
    t._fq_resident = handle
    t._fq_resident_version = t._version
    return t


def resident_of(x):
    """The integer form of an activation, if it has one (a handle, or an fp32 tensor carrying one that is still current)."""
    if type(x) is QHandle:
        return x
    if type(x) in (DeferredConv, DeferredUpsample, DeferredConcat):
        out = x.materialise()
        return out if type(out) is QHandle else None         # (an upsampled int16 sum has the fp32 form only)
    h = getattr(x, "_fq_resident", None)
    if h is not None and getattr(x, "_fq_resident_version", None) != x._version:
        return None                                          # written to since its producer attached the integers
    return h


def as_f32(x):
    return x.to_f32() if type(x) in (QHandle, DeferredConv, DeferredUpsample, DeferredConcat) else x


class Plan(object):
    """What one producer emits.  Plain data (pickles with the module).  Three fields mean different things for different kinds of
    producer (the fields stay as they are: Plan pickles with models):

    field | producer (switch)                           | meaning
    ------+---------------------------------------------+------------------------------------------------------------------------
    grid  | NewAdd                                      | grid of the exact sum
          | windowed nn.AvgPool2d (avgpool)             | grid of its source
          | table activation (activations)              | grid of its source (the table maps it to bit `narrow_bit`)
          | bilinear upsampling (bilinear)              | grid of its source
          | re-quantising Concat (requant)              | the TUPLE of its operands' planned grids, which marks the plan as that
          |                                             | kind (to bit `narrow_bit`)
    up    | nearest upsampling (concat)                 | its factor (with `defer`: the Concat applies it -- or, with topdown, the
          |                                             | NewAdd)
          | bilinear upsampling (bilinear)              | its factor, from grid `grid` to bit `narrow_bit`
          | nn.PixelShuffle / nn.PixelUnshuffle         | its factor r (with `perm`)
          | (pixelshuffle)                              |
    perm  | nn.ChannelShuffle / Slice (shuffle)         | (c_off, C, groups) of fq_shuffle_i8_nhwc
          | nn.PixelShuffle / nn.PixelUnshuffle         | ("d2s", C) / ("s2d", C) of fq_pixel_shuffle_i8_nhwc, C the channels of
          | (pixelshuffle)                              | the shallow tensor
    """
    __slots__ = ("relu", "emit_f32", "emit_int", "narrow_bit", "want_wide", "grid", "resident_add", "defer", "fuse_arg",
                 "fuse_next", "narrow_to_hbm", "fuse_proj", "depthwise", "up", "grouped", "clip", "perm", "table")

    def __init__(self):
        self.relu = False            # the nn.ReLU that consumes this output is fused
        self.emit_f32 = True         # some consumer needs the fp32 NCHW tensor
        self.emit_int = False        # some consumer reads the integer form
        self.narrow_bit = None       # NewAdd: Quantity bit of the conv consumers (None: no narrow output)
        self.want_wide = False       # NewAdd: exact int16 sum needed (next add, or fp32 via dequant)
        self.grid = None             # a grid, by kind of producer: the table above
        self.resident_add = False    # NewAdd: operands arrive as integers
        self.defer = False           # NewConv2d: only consumer is a resident NewAdd, which runs this conv itself
        self.fuse_arg = None         # NewAdd: operand position (0 / 1) that arrives as a DeferredConv
        self.fuse_next = None        # NewAdd: the 1x1 NewConv2d consuming this sum that runs inside the add's kernel too
        self.narrow_to_hbm = True    # NewAdd with fuse_next: somebody besides that convolution reads the int8 re-quantisation
        self.fuse_proj = False       # NewAdd with fuse_arg: the OTHER operand is a deferred 1x1 projection that the kernel computes too
        self.depthwise = False       # NewConv2d: a depthwise layer taken by enable(depthwise=True); runs on fq_dwconv2d_i8_resident
        self.up = None               # a factor, by kind of producer: the table above
        self.grouped = False         # NewConv2d: a grouped layer taken by enable(grouped=True); runs on fq_gconv2d_i8_resident
        self.clip = False            # NewConv2d with `relu`: the fused activation is an nn.ReLU6 (enable(relu6=True)): clipped at 6
        self.perm = None             # a permutation, by kind of producer: the table above
        self.table = None            # elementwise activation taken by enable(activations=True): the 256 int8 of fq_act_lut_i8_nhwc, from grid `grid` to bit `narrow_bit`

    def __getstate__(self):
        return {k: getattr(self, k) for k in self.__slots__}

    def __setstate__(self, state):
        self.__init__()
        for k, v in state.items():
            setattr(self, k, v)

    def sum_outputs(self):
        """(want_wide, want_narrow) of a NewAdd's kernel: the re-quantisation where a convolution reads it, the exact sum where
        somebody needs it or nothing else would be written."""
        want_narrow = self.emit_int and self.narrow_bit is not None
        return self.want_wide or not want_narrow, want_narrow

    def __repr__(self):
        return "Plan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


class _InstanceForward(object):
    """What enable() puts in a module's own `forward` attribute, in front of its class's method; disable() takes it out."""

    def __init__(self, module):
        self.module = module


class _ReluPassThrough(_InstanceForward):
    """Instance-level forward of an nn.ReLU (or, with enable(relu6=True), an nn.ReLU6) whose producer already applied it."""

    def __call__(self, x):
        if type(x) in (QHandle, DeferredConcat):
            if not x.relu_done:
                raise _native.FqError("resident activation reached a ReLU that its producer did not fuse "
                                      "(dataflow changed since resident.enable(); call it again)")
            return x
        if getattr(x, "_fq_relu_done", False):
            return x
        return type(self.module).forward(self.module, x)


class _UnaryResident(_InstanceForward):
    """Instance-level forward of a module with one operand that runs on the integers where it can.  The module needs its plan and
    an operand with an exact 4-D payload of one of `dtypes` -- not a lossy one unless `lossy_source` --; an operand that arrives
    deferred is materialised first (resident_of).  run() then returns what the module hands out, or None; on None, and on every
    miss above, the module's own forward runs on the fp32 form."""
    dtypes = (torch.int8,)           # payloads the kernel reads
    lossy_source = True              # a lossy source is taken (pure data movement and max: Quantity_b commutes with them)

    def __call__(self, x):
        m = self.module
        plan = m.__dict__.get("_resident")
        h = resident_of(x)
        out = None
        if (plan is not None and h is not None and h.exact is not None and h.exact.dtype in self.dtypes and h.exact.dim() == 4
                and (self.lossy_source or not h.lossy)):
            out = self.run(m, plan, h)
        return type(m).forward(m, as_f32(x)) if out is None else out

    def run(self, m, plan, h):
        raise NotImplementedError


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _pointwise(kernel, stride, padding, any_stride=False):
    """A 1x1 convolution without padding at stride 1 -- or, with `any_stride` (a projection shortcut), at any square stride."""
    st = _pair(stride)
    return _pair(kernel) == (1, 1) and _pair(padding) == (0, 0) and (st[0] == st[1] if any_stride else st == (1, 1))


def _pointwise_conv(k, any_stride=False):
    return _pointwise(k.kernel_size, k.stride, k.padding, any_stride)


def _maxpool_supported(m):
    k, st, pd = _pool_geometry(m)
    return (_pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices and 2 * pd[0] <= k[0] and 2 * pd[1] <= k[1]
            and min(st) >= 1)


def _avgpool_is_global(m, h, w):
    """The pool covers the whole h x w plane, and a plane's sum of int16 values stays exact in fp32."""
    return (_pair(m.kernel_size) == (int(h), int(w)) and _pair(m.padding) == (0, 0) and _avgpool_window_ok(m)
            and h * w * 32768 < (1 << 24))


class _MaxPoolResident(_UnaryResident):
    """Instance-level forward of an nn.MaxPool2d between integer layers: pooling the int8 NHWC integers is
    pooling the values (max commutes with the monotone scale q -> q * 2^-g)."""

    def run(self, m, plan, h):
        if not _maxpool_supported(m):
            return None
        return _emit(plan, _moved_handle(h, _native.maxpool_i8_nhwc(h.exact, *_pool_geometry(m)), h.shape[1]))


class _AvgPoolResident(_InstanceForward):
    """Instance-level forward of an nn.AvgPool2d that covers the whole plane of a resident activation."""

    def __call__(self, x):
        m = self.module
        h = resident_of(x)
        if h is not None and h.exact is not None and not h.lossy and _avgpool_is_global(m, h.exact.shape[1], h.exact.shape[2]):
            return _native.avgpool_global_nhwc(h.exact, h.grid, h.shape[1])
        return type(m).forward(m, as_f32(x))


class _AvgPoolWindowResident(_UnaryResident):
    """Instance-level forward of a windowed nn.AvgPool2d between an int8 activation and the convolution(s) behind it
    (enable(avgpool=True)): DeQuantity -> pool -> ReLU -> the consumers' Quantity in one kernel (fq_avgpool_i8_nhwc).  With
    enable(avgpool=True, sums=True) the source may be the exact int16 sum of a NewAdd on the planned grid: that payload goes to
    fq_avgpool_i16_nhwc, the same rule with int32 window sums; a ReLU between sum and pool is the add's fused one
    (h.relu_done), one behind the pool is plan.relu.  The result has no exact integer form: the handle carries the narrow payload
    only, and anything but a NewConv2d at that bit that touches it raises (QHandle.to_f32).  Every run-time miss falls back to the
    module's own forward on the fp32 form."""

    dtypes = (torch.int8, torch.int16)
    lossy_source = False

    def run(self, m, plan, h):
        if plan.narrow_bit is None or plan.grid is None or h.grid != plan.grid or not _avgpool_window_ok(m):
            return None
        k, st, pd = _pool_geometry(m)
        hh, ww = int(h.exact.shape[1]), int(h.exact.shape[2])
        wide = h.exact.dtype == torch.int16                 # a NewAdd's exact sum (planned with sums=True)
        supported, launch = ((_native.avgpool_i16_supported, _native.avgpool_i16_nhwc) if wide else
                             (_native.avgpool_supported, _native.avgpool_i8_nhwc))
        if (not supported(k, st, pd, plan.narrow_bit - h.grid) or hh + 2 * pd[0] < k[0] or ww + 2 * pd[1] < k[1]):
            return None
        y = launch(h.exact, h.shape[1], k, st, pd, m.count_include_pad, plan.narrow_bit - h.grid, plan.relu)
        return QHandle.wide_narrow(h.shape[1], None, None, y, plan.narrow_bit, plan.relu or h.relu_done)


def _shuffle_geometry(m, channels):
    """(c_off, C, groups) of fq_shuffle_i8_nhwc for an nn.ChannelShuffle or a Slice marker that reads `channels` channels, or
    None: groups that is no positive int or does not divide the channels; start / stop that are no plain ints or do not satisfy
    0 <= start < stop <= channels."""
    def plain(v):
        return type(v) is int
    if isinstance(m, nn.ChannelShuffle):
        g = m.groups
        return (0, int(channels), g) if plain(g) and g >= 1 and channels % g == 0 else None
    a, b = getattr(m, "start", None), getattr(m, "stop", None)
    return (a, b - a, 1) if plain(a) and plain(b) and 0 <= a < b <= channels else None


class _ShuffleResident(_UnaryResident):
    """Instance-level forward of an nn.ChannelShuffle between integer layers (enable(shuffle=True)): permuting the channels of
    the int8 NHWC integers is permuting the values (fq_shuffle_i8_nhwc).  Whenever a run-time condition fails -- no plan, no int8
    exact payload, a geometry other than the planned one -- the module's own forward runs on the fp32 form."""

    def run(self, m, plan, h):
        geo = _shuffle_geometry(m, h.shape[1])
        if geo is None or geo != plan.perm or not _native.shuffle_supported(h.shape[1], *geo):
            return None
        c_off, c, g = geo
        return _emit(plan, _moved_handle(h, _native.shuffle_i8_nhwc(h.exact, h.shape[1], c_off, c, g), c))


class _SliceResident(_ShuffleResident):
    """Instance-level forward of a Slice marker between integer layers (enable(shuffle=True)): channels [start, stop) of the int8
    NHWC integers as a tensor of their own, the padding channels zero (fq_shuffle_i8_nhwc with one group)."""


PIXEL_FACTORS = (2, 3, 4)          # the factors fq_pixel_shuffle_i8_nhwc takes


def _pixel_factor(m):
    """The factor of an nn.PixelShuffle / nn.PixelUnshuffle as the module holds it (any object)."""
    return m.upscale_factor if isinstance(m, nn.PixelShuffle) else m.downscale_factor


def _pixel_geometry(m, shape):
    """(r, ("d2s" | "s2d", C)) -- Plan.up and Plan.perm -- of fq_pixel_shuffle_i8_nhwc for an nn.PixelShuffle / nn.PixelUnshuffle that
    reads a 4-D activation of `shape` (N, channels, height, width), C the channels of the shallow tensor; or None: a factor that is
    no plain int of PIXEL_FACTORS, channels that r^2 does not divide (a shuffle), a plane that r does not divide (an unshuffle)."""
    r = _pixel_factor(m)
    if type(r) is not int or r not in PIXEL_FACTORS or len(shape) != 4:
        return None
    channels, hh, ww = int(shape[1]), int(shape[2]), int(shape[3])
    if isinstance(m, nn.PixelShuffle):
        return (r, ("d2s", channels // (r * r))) if channels % (r * r) == 0 and channels >= r * r else None
    return (r, ("s2d", channels)) if hh % r == 0 and ww % r == 0 and hh >= r and ww >= r else None


class _PixelShuffleResident(_UnaryResident):
    """Instance-level forward of an nn.PixelShuffle / nn.PixelUnshuffle between integer layers (enable(pixelshuffle=True)):
    permuting the int8 NHWC integers between depth and space is permuting the values (fq_pixel_shuffle_i8_nhwc).  The handle is
    built as _ShuffleResident builds its own (_moved_handle).  Whenever a run-time condition fails -- no plan, no int8 exact
    payload, a factor, direction or width other than the planned one, a geometry the kernel refuses -- the module's own forward
    runs on the fp32 form."""

    def run(self, m, plan, h):
        geo = _pixel_geometry(m, (h.shape[0], h.shape[1], h.exact.shape[1], h.exact.shape[2]))
        if geo is None or geo != (plan.up, plan.perm) or not _native.pixel_shuffle_supported(geo[1][1], geo[0], geo[1][0] == "s2d"):
            return None
        r, (way, c) = geo
        y = _native.pixel_shuffle_i8_nhwc(h.exact, c, r, way == "s2d")
        return _emit(plan, _moved_handle(h, y, c if way == "d2s" else c * r * r))


ACTIVATION_TYPES = (nn.LeakyReLU, nn.PReLU, nn.Hardswish, nn.Hardsigmoid, nn.SiLU, nn.Sigmoid, nn.Tanh, nn.ELU, nn.Hardtanh, nn.Mish,
                    nn.GELU)


def _is_table_activation(m):
    """An elementwise activation module that enable(activations=True) hooks.  nn.ReLU and nn.ReLU6 (a subclass of nn.Hardtanh)
    keep their own paths: they are clamps, fused as an Sp range."""
    return isinstance(m, ACTIVATION_TYPES) and not isinstance(m, (nn.ReLU, nn.ReLU6))


class _ActTableResident(_UnaryResident):
    """Instance-level forward of an elementwise activation between integer layers (enable(activations=True)): the int8 NHWC
    integers on the planned grid go through the module's 256-entry table (fq_act_lut_i8_nhwc) and come out as the integers the
    convolutions behind it would quantise to.  The handle is marked `lossy`: it stands for Quantity_b(f(x)), not for f(x).
    Whenever a run-time condition fails -- no plan, no int8 exact payload, another grid than the planned one -- the module's own
    forward runs on the fp32 form."""

    lossy_source = False

    def run(self, m, plan, h):
        if plan.table is None or h.grid != plan.grid or not _native.act_lut_supported(h.shape[1]):
            return None
        return _emit(plan, _lossy_int8(_native.act_lut_i8_nhwc(h.exact, h.shape[1], plan.table), h.shape[1], plan.narrow_bit, False))


def _pool_geometry(m):
    return _pair(m.kernel_size), _pair(m.stride if m.stride is not None else m.kernel_size), _pair(m.padding)


def _avgpool_window_ok(m):
    return not m.ceil_mode and getattr(m, "divisor_override", None) is None


def _upsample_factor(m):
    """2 or 4 for an nn.Upsample / nn.UpsamplingNearest2d that fq_concat_i8_nhwc can stand for: mode "nearest", no `size`, one
    integer scale factor for both axes; None for anything else."""
    if not isinstance(m, nn.Upsample) or m.mode != "nearest" or m.size is not None or m.scale_factor is None:
        return None
    sf = m.scale_factor
    if isinstance(sf, (tuple, list)):
        if len(sf) != 2 or sf[0] != sf[1]:
            return None
        sf = sf[0]
    return int(sf) if float(sf) in (2.0, 4.0) else None


def _bilinear_factor(m):
    """2 or 4 for an nn.Upsample that fq_upsample_bilinear_i8_nhwc can stand for: mode "bilinear", align_corners false, no `size`,
    one integer scale factor for both axes; None for anything else (_bilinear_form_left says which)."""
    return None if _bilinear_form_left(m) is not None else int(_scale_factor(m))


def _scale_factor(m):
    sf = m.scale_factor
    if isinstance(sf, (tuple, list)):
        return sf[0] if len(sf) == 2 and sf[0] == sf[1] else None
    return sf


def _bilinear_form_left(m):
    """Why a bilinear-mode nn.Upsample is no module of enable(bilinear=True) by its own arguments, or None."""
    if not isinstance(m, nn.Upsample) or m.mode != "bilinear":
        return "no bilinear-mode nn.Upsample"
    if m.align_corners:
        return "align_corners=True: its weights are no dyadic numbers, the integer rule is not exact (fp32 form)"
    if m.size is not None or m.scale_factor is None:
        return "the `size=` form: only an integer scale_factor is taken (fp32 form)"
    sf = _scale_factor(m)
    if sf is None or float(sf) not in (2.0, 4.0):
        return "scale_factor %r: only one integer factor of 2 or 4 for both axes is taken (fp32 form)" % (m.scale_factor,)
    return None


def _emit(plan, out, t=None):
    """A finished integer activation as its consumers want it: the handle, or the fp32 tensor (carrying the handle where
    somebody reads the integers too).  The only copy of this hand-off: every integer producer ends here.  plan None: a layer
    switched per instance, outside a plan, hands out the plain fp32 tensor.  t: the fp32 tensor, where the producer's kernel
    wrote it itself."""
    if plan is not None and not plan.emit_f32:
        return out
    if t is None:
        t = out.to_f32()
    if plan is not None and plan.emit_int:
        carry(t, out)
    if out.relu_done:
        t._fq_relu_done = True
    return t


class _UpsampleResident(_UnaryResident):
    """Instance-level forward of a nearest upsampling between integer layers: repeating the int8 NHWC integers is repeating the
    values.  With plan.defer nothing runs here: the resident Concat that consumes it reads the small tensor (DeferredUpsample)."""

    def run(self, m, plan, h):
        if plan.up is None or plan.up != _upsample_factor(m) or h.grid != plan.narrow_bit:
            return None
        if plan.defer and not plan.relu:
            return DeferredUpsample(h, plan.up)
        y = _native.concat_i8_nhwc([(h.exact, h.shape[1], plan.up)], plan.relu)
        return _emit(plan, _moved(QHandle.int8(y, h.shape[1], h.grid, plan.relu or h.relu_done), h))


class _BilinearResident(_UnaryResident):
    """Instance-level forward of a bilinear upsampling between an int8 activation and the convolutions behind it
    (enable(concat=True, bilinear=True)): DeQuantity -> interpolation -> ReLU -> the consumers' Quantity in one kernel
    (fq_upsample_bilinear_i8_nhwc).  The handle is marked `lossy`: it stands for Quantity_b(up(x)), not for up(x).  Whenever a
    run-time condition fails -- no plan, no int8 exact payload, another grid than the planned one, a lossy source, a factor or shift
    the kernel does not take -- the module's own forward runs on the fp32 form."""

    lossy_source = False

    def run(self, m, plan, h):
        if (plan.up is None or plan.grid is None or plan.narrow_bit is None or plan.up != _bilinear_factor(m)
                or h.grid != plan.grid or not _native.upsample_bilinear_supported(plan.up, plan.narrow_bit - h.grid)):
            return None
        y = _native.upsample_bilinear_i8_nhwc(h.exact, h.shape[1], plan.up, plan.narrow_bit - h.grid, plan.relu)
        return _emit(plan, _lossy_int8(y, h.shape[1], plan.narrow_bit, plan.relu or h.relu_done))


class _UpsampleTopDown(_UnaryResident):
    """Instance-level forward of a nearest upsampling whose readers are resident NewAdds (enable(concat=True, topdown=True)):
    nothing runs here.  The coarse handle -- int8, or the exact int16 sum of the add one level up -- goes to the add as a
    DeferredUpsample, and the add reads it at (h / s, w / s) (fq_add_up_resident).  A run-time miss -- no integer payload on the
    planned grid -- runs the module's own forward on the fp32 form."""

    dtypes = (torch.int8, torch.int16)

    def run(self, m, plan, h):
        if plan.up is None or not plan.defer or plan.up != _upsample_factor(m) or h.grid != plan.narrow_bit:
            return None
        return DeferredUpsample(h, plan.up, m)


class _ConcatResident(_InstanceForward):
    """Instance-level forward of a Concat marker whose operands are int8 NHWC on one grid: concatenating the integers is
    concatenating the values (fq_concat_i8_nhwc, the nn.ReLU behind it fused).  An operand that arrives as a DeferredUpsample is
    upsampled by the same kernel; one that arrives as a DeferredConcat (enable(flatten=True)) is expanded into its leaves, and the
    whole list goes out in one launch (_concat_launch).  With plan.defer nothing runs here either: the leaves are handed on."""

    @staticmethod
    def _leaves(operands, expand):
        out = []
        for t in operands:
            if expand and type(t) is DeferredConcat and t._out is None:
                out.extend(t.leaves)
            elif type(t) is DeferredUpsample and t._out is None:
                out.append((t.handle, t.s, False))
            else:
                out.append((resident_of(t), 1, False))
        return out

    @staticmethod
    def _fits(plan, dim, leaves):
        ok = plan is not None and dim == 1 and len(leaves) <= MAX_CONCAT_LEAVES
        for h, _up, _r in leaves:
            ok = ok and h is not None and h.exact is not None and h.exact.dtype == torch.int8 and h.exact.dim() == 4 \
                and h.grid == plan.narrow_bit
        if ok:
            planes = set((h.exact.shape[0], h.exact.shape[1] * up, h.exact.shape[2] * up) for h, up, _r in leaves)
            supported = _native.concat_supported if len(leaves) <= 2 else _native.concat_n_supported
            ok = len(planes) == 1 and supported([h.shape[1] for h, _up, _r in leaves], [up for _h, up, _r in leaves])
        return ok

    def __call__(self, x, y, dim=1):
        m = self.module
        plan = m.__dict__.get("_resident")
        leaves = self._leaves((x, y), True)
        ok = self._fits(plan, dim, leaves)
        if not ok and any(type(t) is DeferredConcat and t._out is None for t in (x, y)):
            leaves = self._leaves((x, y), False)            # the deferred parts are materialised: the two-operand path
            ok = self._fits(plan, dim, leaves)
        if not ok:
            return type(m).forward(m, as_f32(x), as_f32(y), dim)
        if plan.relu:
            leaves = [(h, up, True) for h, up, _r in leaves]
        if plan.defer:
            return DeferredConcat(leaves, plan.narrow_bit)
        q = _concat_launch(leaves)
        return _emit(plan, _moved(QHandle.int8(q, sum(h.shape[1] for h, _up, _r in leaves), plan.narrow_bit,
                                               all(r or h.relu_done for h, _up, r in leaves)), *[h for h, _up, _r in leaves]))


class _ConcatRequant(_InstanceForward):
    """Instance-level forward of a Concat marker that re-quantises (enable(concat=True, requant=True)): its operands lie on
    their own grids -- int8 activations, directly or through a deferred nearest upsampling, or the exact int16 sum of a resident
    NewAdd -- and every reader quantises at one bit b = plan.narrow_bit, so DeQuantity_g -> cat -> (ReLU) -> Quantity_b runs as one
    kernel on the integers (fq_concat_rq_i8_nhwc), each source shifted by b - its handle's grid.  plan.grid holds the tuple of the
    planned operand grids and marks the plan as this kind.  The handle is `lossy`: it stands for Quantity_b(cat(...)).  A lossy
    operand (a table activation, a bilinear upsampling, another such Concat) is taken at bit b only: its integers are copied.
    Every run-time miss -- no exact payload, a lossy operand at another bit, planes that differ, a geometry or shift the kernel
    does not take -- runs the marker's own forward on the fp32 forms (which raises where an operand has none)."""

    @staticmethod
    def _sources(plan, dim, operands):
        if plan is None or type(plan.grid) is not tuple or plan.narrow_bit is None or dim != 1:
            return None
        b, out = plan.narrow_bit, []
        for t in operands:
            if type(t) is DeferredUpsample and t._out is None and t.handle.exact is not None and t.handle.exact.dtype == torch.int8:
                h, up = t.handle, t.s
            else:
                h, up = resident_of(t), 1
            if (h is None or h.exact is None or h.exact.dim() != 4 or h.exact.dtype not in (torch.int8, torch.int16)
                    or (h.lossy and (h.grid != b or h.exact.dtype != torch.int8))):
                return None
            out.append((h, up))
        planes = set((h.exact.shape[0], h.exact.shape[1] * up, h.exact.shape[2] * up) for h, up in out)
        if len(planes) != 1 or not _native.concat_rq_supported([h.shape[1] for h, _up in out], [up for _h, up in out],
                                                               [h.exact.element_size() for h, _up in out],
                                                               [b - h.grid for h, _up in out]):
            return None
        return out

    def __call__(self, x, y, dim=1):
        m = self.module
        plan = m.__dict__.get("_resident")
        srcs = self._sources(plan, dim, (x, y))
        if srcs is None:
            return type(m).forward(m, as_f32(x), as_f32(y), dim)
        b = plan.narrow_bit
        q = _native.concat_rq_i8_nhwc([(h.exact, h.shape[1], up, plan.relu, b - h.grid) for h, up in srcs])
        return _emit(plan, _lossy_int8(q, sum(h.shape[1] for h, _up in srcs), b, plan.relu or all(h.relu_done for h, _up in srcs)))


# ---- tracing -------------------------------------------------------------------------------------

class _Value(object):
    __slots__ = ("producer", "kind", "src", "consumers", "foreign", "shape")

    def __init__(self, producer, kind, src):
        self.producer, self.kind, self.src = producer, kind, src
        self.shape = None            # shape of the traced tensor (set when the value is recorded)
        self.consumers = []          # (module, argument position)
        self.foreign = False         # touched by code outside NewConv2d / NewLinear / NewAdd / nn.ReLU


def _iter_tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            for t in _iter_tensors(o):
                yield t
    elif isinstance(obj, dict):
        for o in obj.values():
            for t in _iter_tensors(o):
                yield t


class _Tracer(TorchFunctionMode):

    def __init__(self, avgpool=False):
        super(_Tracer, self).__init__()
        self.avgpool = bool(avgpool)     # enable(avgpool=True): an nn.AvgPool2d output is a traced value
        self.seen = collections.defaultdict(list)    # report attribute of _KINDS -> every hooked module that reports there, in execution order
        self.inplace = set()             # hooked modules that returned their own input tensor
        self.values = {}             # id(tensor) -> _Value
        self.keep = []               # keeps traced tensors alive so ids are not reused
        self.depth = 0
        self.calls = {}              # module -> number of forward calls
        self.produced = []           # _Value of every NewConv2d / NewAdd output, in execution order
        self.relu_values = []        # _Value of every nn.ReLU output whose input is traced
        self.avgpool_shapes = {}     # nn.AvgPool2d module -> shape of its (traced) input
        self.concat_ok = {}          # Concat module -> every call so far joined two 4-D tensors along dim 1

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if self.depth == 0:
            self.mark_foreign((args, kwargs))
        return func(*args, **kwargs)

    # module hooks
    def pre(self, module, args):
        self.depth += 1
        self.calls[module] = self.calls.get(module, 0) + 1
        report = _row(module).report
        if report is not None and module not in self.seen[report]:
            self.seen[report].append(module)
        for pos, a in enumerate(args):
            v = self.values.get(id(a)) if isinstance(a, torch.Tensor) else None
            if v is not None:
                v.consumers.append((module, pos))
                if isinstance(module, nn.AvgPool2d) and pos == 0:
                    self.avgpool_shapes[module] = tuple(a.shape)       # (depth > 0 here: not a foreign touch)

    def pre_concat(self, module, args, kwargs):
        """Pre-hook of a Concat marker (with_kwargs: `dim`, and the operands themselves, may be given by name)."""
        named = [kwargs[k] for k in ("x", "y") if k in kwargs]
        self.pre(module, tuple(args[:2]) + tuple(named))
        dim = args[2] if len(args) > 2 else kwargs.get("dim", 1)
        pair = (tuple(args[:2]) + tuple(named))[:2]
        ok = (isinstance(dim, int) and dim == 1 and len(pair) == 2
              and all(isinstance(t, torch.Tensor) and t.dim() == 4 for t in pair))
        self.concat_ok[module] = ok and self.concat_ok.get(module, True)

    @staticmethod
    def _kind(module):
        return _row(module).name

    def post(self, module, args, output):
        self.depth -= 1
        if not isinstance(output, torch.Tensor):
            return
        row = _row(module)
        kind = row.name
        src = None
        if args and output is args[0]:
            self.inplace.add(module)
        if row.behind:                                      # a value of these kinds exists only behind a traced value
            if kind == "avgpool" and not self.avgpool:
                return                                      # its output is an ordinary fp32 tensor
            src = self.values.get(id(args[0])) if args and isinstance(args[0], torch.Tensor) else None
            if src is None:
                return
            if kind == "avgpool" and (src.shape is None or len(src.shape) != 4):    # (the recorded shape: a tensor method here would be a foreign touch)
                return
        v = _Value(module, kind, src)
        (self.relu_values if kind == "relu" else self.produced).append(v)
        v.shape = tuple(output.shape)
        self.values[id(output)] = v
        self.keep.append(output)

    def mark_foreign(self, obj):
        for t in _iter_tensors(obj):
            v = self.values.get(id(t))
            if v is not None:
                v.foreign = True


def _clear(model):
    for m in model.modules():
        m.__dict__.pop("_resident", None)
        fwd = m.__dict__.get("forward")
        if isinstance(fwd, _InstanceForward):
            del m.__dict__["forward"]
    for key in [k for k in model.__dict__ if k.startswith("_fq_resident_")]:     # (the per-switch keys of earlier versions too)
        del model.__dict__[key]


def disable(model):
    """Back to the reference's fp32 module boundaries."""
    _clear(model)
    return model


def is_enabled(model):
    return bool(model.__dict__.get("_fq_resident_enabled"))


# enable()'s opt-in switches: (name, the summary keys it adds, the report attributes of describe() it fills), in the order in
# which the keys enter the summary behind the six base keys (tests compare key lists)
_SWITCH_TABLE = (
    ("depthwise", ("resident_depthwise",), ()),
    ("concat", ("resident_concats", "resident_upsamples"), ()),
    ("flatten", ("flattened_concats",), ()),
    ("avgpool", ("resident_avgpools",), ()),
    ("sums", ("resident_sum_avgpools",), ("avgpool_left",)),
    ("grouped", ("resident_grouped",), ()),
    ("relu6", ("fused_relu6s",), ("relu6_left",)),
    ("shuffle", ("resident_shuffles", "resident_slices"), ("shuffle_left",)),
    ("activations", ("resident_activations",), ("activations_left",)),
    ("topdown", ("topdown_adds", "topdown_sum_sources"), ("topdown_left",)),
    ("bilinear", ("resident_bilinears",), ("bilinear_left",)),
    ("requant", ("requant_concats", "requant_sum_sources"), ("requant_left",)),
    ("pixelshuffle", ("resident_pixelshuffles", "resident_pixelunshuffles"), ("pixelshuffle_left",)),
    ("deconv", ("resident_deconvs",), ("deconv_left",)),
)
_Switches = collections.namedtuple("_Switches", [name for name, _keys, _reports in _SWITCH_TABLE])
# (switch, the switch it needs, enable()'s ValueError without it)
_SWITCH_NEEDS = (
    ("flatten", "concat", "resident.enable(flatten=True) needs concat=True: only planned Concats are flattened"),
    ("sums", "avgpool", "resident.enable(sums=True) needs avgpool=True: only planned windowed pools read a NewAdd sum"),
    ("topdown", "concat", "resident.enable(topdown=True) needs concat=True: the upsampling is hooked by that switch"),
    ("bilinear", "concat", "resident.enable(bilinear=True) needs concat=True: the Concat behind a decoder's upsampling is planned by that switch"),
    ("requant", "concat", "resident.enable(requant=True) needs concat=True: only a hooked Concat marker re-quantises"),
)


def _switches(**on):
    """The switches of one enable() call as an immutable record: every one named in `on` by its truth value, the rest off."""
    return _Switches(**dict((name, bool(on.pop(name, False))) for name in _Switches._fields), **on)     # (an unknown name: TypeError)


class _Planning(object):
    """The plan of one traced forward.  enable() calls the passes below in order; they decide on the trace alone and change
    nothing on the model until install() writes the plans and the instance-level forwards to the modules."""

    def __init__(self, tracer, switches, revoked=None, names=None):
        from .new_quantity_op import NewConv2d, NewAdd, NewConvTranspose2d
        from .fabu_layer import Concat
        self.conv_type, self.concat_type, self.deconv_type = NewConv2d, Concat, NewConvTranspose2d
        self.tracer = tracer
        self.sw = switches               # the _Switches of this enable() call
        self.revoked = dict(revoked or {})   # module that an earlier round planned and verify() took back -> why
        self.names = names or {}         # module -> its name in the model (for the reasons)
        self.left = collections.defaultdict(dict)    # report attribute of describe() -> {module that stays torch's: why}
        self.fields = {}                 # module -> the Plan fields that its format rule decided
        self.forward_of = {}             # module -> its instance-level forward, where that is not its kind's
        self.lossy = {}                  # planned table activation, bilinear upsampling or re-quantising Concat -> its readers' bit b
        self.value_of = dict((v.producer, v) for v in tracer.produced)
        self.relu_value = dict((id(c.src), c) for c in tracer.relu_values)
        self.fmt = {}                    # id(effective _Value) -> (bytes, grid)
        self.eff_of = {}                 # id(produced _Value) -> (effective _Value, relu module)
        self.operands = {}               # NewAdd / Concat module -> [value at arg 0, value at arg 1]
        for v in tracer.values.values():
            for (m, pos) in v.consumers:
                if isinstance(m, (NewAdd, Concat)) and pos < 2:
                    self.operands.setdefault(m, [None, None])[pos] = v
        self.add_resident = set()        # NewAdd modules whose operands arrive as integers
        self.int8_resident = set()       # nn.MaxPool2d, Concat, nearest-upsampling, nn.ChannelShuffle, Slice and nn.PixelShuffle / nn.PixelUnshuffle modules that run on the int8 integers
        self.avg_resident = {}           # windowed nn.AvgPool2d that runs on fq_avgpool_i8_nhwc -> (source grid g, consumer bit b)
        self.avg_sum = set()             # (avgpool=True, sums=True) the pools of avg_resident that read a NewAdd's exact int16 sum (fq_avgpool_i16_nhwc)
        self.topdown_ups = {}            # (concat=True, topdown=True) upsampling that a NewAdd reads at (h / s, w / s) -> (bytes, grid) of its source
        self.topdown_adds = set()        # ... the NewAdd modules that take such an operand
        self.rq_cats = set()             # (concat=True, requant=True) the planned Concats that re-quantise their operands (fq_concat_rq_i8_nhwc)
        self.plans = {}                  # producer module -> Plan
        self.forwards = []               # (module, its instance-level forward)
        self.summary = {"resident_convs": 0, "resident_adds": 0, "resident_pools": 0, "fused_relus": 0, "fp32_outputs": 0,
                        "int_only_outputs": 0}
        for name, keys, _reports in _SWITCH_TABLE:
            if getattr(switches, name):
                self.summary.update((key, 0) for key in keys)

    # ---- what a value is and what a module can do

    def once(self, m):
        """Every producer of the plan is called exactly once per forward."""
        return self.tracer.calls.get(m, 0) == 1

    def effective(self, v):
        """(value the consumers see, fused ReLU / ReLU6 module or None)"""
        if _KIND[v.kind].fuse_relu and not v.foreign and len(v.consumers) == 1 and isinstance(v.consumers[0][0], (nn.ReLU, nn.ReLU6)):
            act = v.consumers[0][0]
            after = self.relu_value.get(id(v))
            if after is not None and (isinstance(act, nn.ReLU) or self.takes_relu6(v)):
                return after, act
        return v, None

    def takes_relu6(self, v):
        """`relu6=True` fuses an nn.ReLU6 that is the only reader of a NewConv2d's output like an nn.ReLU: the producer (dense,
        stem, depthwise with `depthwise=True`, grouped with `grouped=True`) clamps its integers to [0, 6 * 2^output_bit]
        (fq_*_act, _native.relu6_clip; from output_bit = 5 on that is the plain fused ReLU).  Not taken, and left to torch on the
        fp32 tensor exactly as without the argument: a layer with output_bit <= -2 (6 is not on its output grid), a producer
        that is no integer convolution of this plan, and a ReLU6 behind a NewAdd, a Concat, a pool or an upsampling.  16-bit
        models have no plan at all.  The summary then gains `fused_relu6s`; describe() names what was left."""
        m = v.producer
        if not self.sw.relu6 or v.kind != "contraction" or not self.conv_can_emit(m):
            return False
        return _native.relu6_clip(m.output_bit) is not None

    def _relu6_reasons(self):
        """Why each hooked nn.ReLU6 that no producer fused stays torch's (for describe())."""
        fused = set(m for (m, forward) in self.forwards if isinstance(forward, _ReluPassThrough))
        source = {}
        for r in self.tracer.relu_values:
            source.setdefault(r.producer, r.src)
        for act in self.tracer.seen["relu6_left"]:
            if act in fused:
                continue
            v = source.get(act)
            if v is None:
                why = "its input is not the output of a planned layer"
            elif v.kind != "contraction":
                why = "behind %s: only a ReLU6 behind a convolution is fused" % {"add": "a NewAdd", "concat": "a Concat"}.get(
                    v.kind, "a pool or an upsampling")
            elif not self.conv_can_emit(v.producer):
                why = "its producer is not an integer convolution of this plan (fp32 form)"
            elif _native.relu6_clip(v.producer.output_bit) is None:
                why = "output_bit %d <= -2: the value 6 is not on the output grid (fp32 form)" % v.producer.output_bit
            elif v.foreign or len(v.consumers) != 1:
                why = "the convolution's output has other readers"
            else:
                why = "the ReLU6 was called more than once"
            self.left["relu6_left"][act] = why

    def is_dw(self, m):
        """A depthwise layer that this plan runs on fq_dwconv2d_i8_resident: `depthwise=True` plans depthwise NewConv2d layers
        (groups == in_channels == out_channels, 3x3 / 5x5, stride 1 / 2, shift in [1, 16]: NewConv2d._depthwise_ok) as integer
        producers and consumers; without it they stay fp32 producers, as every other grouped convolution does.  The summary then
        counts them as `resident_depthwise`."""
        return self.sw.depthwise and isinstance(m, self.conv_type) and self.once(m) and m._depthwise_ok(m.Conv, True)

    def is_gc(self, m):
        """A grouped layer that this plan runs on fq_gconv2d_i8_resident: `grouped=True` plans grouped NewConv2d layers
        (1 < groups < channels, 4 .. 64 input and output channels per group in multiples of 4, 1x1 / 3x3, stride 1 / 2, shift in
        [1, 16]: NewConv2d._grouped_ok) as integer producers and consumers.  Such a layer is never run inside a NewAdd's kernel;
        an add reads its integers like any other operand.  Without the argument they stay fp32 producers.  The summary then counts
        them as `resident_grouped`."""
        return self.sw.grouped and isinstance(m, self.conv_type) and self.once(m) and m._grouped_ok(m.Conv, True)

    def is_dc(self, m):
        """A transposed convolution that this plan runs on fq_deconv2d_i8_resident: `deconv=True` plans NewConvTranspose2d layers
        (groups 1, dilation 1, kernel 1 .. 8, stride 1 .. 4, zero padding below the kernel size, output_padding below the stride,
        shift in [1, 16], per-tensor bits: NewConvTranspose2d._deconv_ok) as integer producers at their output_bit and integer
        consumers at their input_bit, the third own-kernel family beside depthwise and grouped.  An nn.ReLU behind one is fused,
        with `relu6=True` an nn.ReLU6 as well; wherever a lossy value (a table activation, a bilinear upsampling, a re-quantising
        Concat) requires integer convolutions at one bit of its readers, it is one.  Such a layer is never run inside a NewAdd's
        kernel and never part of a block tail or a fused projection; an add reads its integers like any other operand.  Without
        the argument it stays an fp32 producer, as a grouped convolution does without `grouped=True`.  The summary then counts
        them as `resident_deconvs`; describe().deconv_left names the ones left with the reason: groups, dilation, a geometry or
        shift the kernel refuses, called more than once."""
        return self.sw.deconv and isinstance(m, self.deconv_type) and self.once(m) and m._deconv_ok(m.Conv, True)

    def conv_can_emit(self, m):
        if isinstance(m, self.deconv_type):
            return self.is_dc(m)
        return isinstance(m, self.conv_type) and self.once(m) and (m._int8_ok(m.Conv) or self.is_dw(m) or self.is_gc(m))

    def conv_can_read(self, m):
        if isinstance(m, self.deconv_type):
            return self.is_dc(m)
        return isinstance(m, self.conv_type) and ((m._int8_ok(m.Conv) and not m._stem_fold(m.Conv)) or self.is_dw(m)
                                                  or self.is_gc(m))

    def _deconv_reasons(self):
        """Why each traced NewConvTranspose2d without a plan stays an fp32 producer (for describe().deconv_left)."""
        for m in self.tracer.calls:
            if isinstance(m, self.deconv_type) and m not in self.plans:
                self.left["deconv_left"][m] = ("the module was called more than once" if not self.once(m)
                                               else m._deconv_left(m.Conv) or "its output has no integer form in this plan")

    def avg_can_read(self, m):
        """The whole-plane nn.AvgPool2d in front of the head, which reads the exact integers of its source (_AvgPoolResident)."""
        shape = self.tracer.avgpool_shapes.get(m)
        return isinstance(m, nn.AvgPool2d) and shape is not None and len(shape) == 4 and _avgpool_is_global(m, shape[2], shape[3])

    def resident_adds(self):
        """(module, its Plan, its two operand values, its own value) of every resident add, in execution order."""
        return [(v.producer, self.plans[v.producer], self.operands[v.producer], v) for v in self.tracer.produced
                if v.kind == "add" and v.producer in self.add_resident]

    # ---- pass 1 (execution order): integer format of every produced value

    def plan_formats(self):
        for v in self.tracer.produced:
            e, relu_mod = self.effective(v)
            self.eff_of[id(v)] = (e, relu_mod)
            row = _KIND[v.kind]
            f = row.rule(self, v)                           # (the rule also notes what else it decided: fields, forward_of, left)
            if f is not None:
                self.fmt[id(e)] = f
                if row.forward is not None:                 # (a module that is no integer layer itself: it runs on its source's int8)
                    self.int8_resident.add(v.producer)

    def _conv_format(self, v):
        """A NewConv2d / NewLinear that this plan runs on integers emits int8 at its own output bit."""
        m = v.producer
        if not self.conv_can_emit(m):
            return None
        if self.is_dw(m):
            self.fields.setdefault(m, {})["depthwise"] = True
            self.summary["resident_depthwise"] += 1
        if self.is_gc(m):
            self.fields.setdefault(m, {})["grouped"] = True
            self.summary["resident_grouped"] += 1
        if self.is_dc(m):
            self.summary["resident_deconvs"] += 1
        return (1, m.output_bit)

    def _int8_source(self, v):
        """The format of the value that a max-pool / upsampling / average pool called once reads, if that is int8."""
        f = self.fmt.get(id(v.src))
        return f if f is not None and f[0] == 1 and self.once(v.producer) else None

    def _maxpool_format(self, v):
        return self._int8_source(v) if _maxpool_supported(v.producer) else None

    def _upsample_format(self, v):
        """A nearest upsampling by 2 or 4 (`concat=True`, _concat_format) repeats the int8 integers of its source; with
        `topdown=True` one in front of a NewAdd launches nothing (_topdown_format)."""
        m = v.producer
        s = _upsample_factor(m)
        f = self._int8_source(v) if s is not None and len(v.shape) == 4 else None
        if f is not None and not _native.concat_supported([v.shape[1]], [s]):
            f = None
        if self.sw.topdown:
            f = self._topdown_format(v, self.eff_of[id(v)][1], f)
        self.fields[m] = {"up": s}
        if m in self.topdown_ups:                           # (nothing is launched: the adds behind it read the coarse tensor)
            self.fields[m].update(defer=True, emit_int=True, emit_f32=False)
            self.forward_of[m] = _UpsampleTopDown
        return f

    def _topdown_format(self, v, relu_mod, f_off):
        """`concat=True, topdown=True` plans a nearest upsampling by 2 or 4 whose readers are NewAdds -- the FPN top-down step
        Eltwise(lateral, up(top)) -- as an operand of those adds: the module launches nothing (Plan.up = s, Plan.defer = True,
        integers only), each add reads the coarse tensor at (h / s, w / s) (fq_add_up_resident) and the upsampled tensor is never
        written.  The source may be an int8 activation (format (1, g)) or the exact int16 sum of a resident NewAdd ((2, g), with
        that add's fused ReLU, if any): nearest upsampling repeats values, so the add's arithmetic is unchanged.  The sum in front
        counts the upsampling as a reader of its exact integers (_readers) and writes no fp32 for it.  Taken when the module is
        called once, every reader is a NewAdd called once and no ReLU sits between the upsampling and the add; verify_topdown()
        then checks the adds.  Returns the format of the upsampled value: the source's when planned, else `f_off`, what the plan
        without the switch gives it, with the reason in topdown_left (describe().topdown_left) where a NewAdd reads it or it
        reads a sum.  Left as they were: `size=` forms, other factors and modes (foreign code: not hooked), a module called
        twice, any reader besides NewAdds, a ReLU behind the upsampling, both operands of an add upsampled, planes the factor
        does not divide.  The summary gains `topdown_adds` and `topdown_sum_sources`."""
        m = v.producer
        src = self.fmt.get(id(v.src))
        root = v.src.src if v.src.kind == "relu" and v.src.src is not None else v.src
        adds = [c for (c, _pos) in v.consumers if self.tracer._kind(c) == "add"]
        behind = self.relu_value.get(id(v))                 # the value of a ReLU that reads the upsampling, if there is one
        relu_adds = [c for (c, _pos) in behind.consumers if self.tracer._kind(c) == "add"] if behind is not None else []
        over_sum = src is not None and src[0] == 2
        if not adds and not relu_adds and not over_sum:
            return f_off                                    # an upsampling in front of a Concat or a convolution: not this switch's
        s = _upsample_factor(m)
        why = None
        if not self.once(m):
            why = "the module was called more than once"
        elif src is None:
            why = "its source has no integer form in this plan (fp32 form)"
        elif over_sum and root.kind != "add":
            why = "its source is int16 but no NewAdd sum (fp32 form)"
        elif len(v.shape) != 4:
            why = "its input is not 4-D"
        elif relu_mod is not None or relu_adds:
            why = "a ReLU sits between the upsampling and the add"
        elif v.foreign or len(adds) != len(v.consumers) or not adds:
            others = [self._name(c) for (c, _pos) in v.consumers if self.tracer._kind(c) != "add"]
            why = "read by %s besides the NewAdd: every reader must be a NewAdd%s" % (
                ", ".join(others) if others else "code outside the plan", " (a sum has no upsampled integer form: fp32 form)" if over_sum else "")
        elif not all(self.once(c) for c in adds):
            why = "a NewAdd that reads it was called more than once"
        elif not _native.add_up_supported(s, v.shape[2], v.shape[3], _native.pad16(v.shape[1])):
            why = "the %dx%d plane is not divisible by the factor %d" % (v.shape[2], v.shape[3], s)
        elif m in self.revoked:
            why = self.revoked[m]
        if why is None:
            self.topdown_ups[m] = src
            return src
        self.left["topdown_left"][m] = why
        return f_off

    def verify_topdown(self):
        """{upsampling: why} for every one planned by _topdown_format whose adds, after all passes, cannot take it: an add that
        is not resident (its other operand has no integer form, or the grid does not fit int16), or one whose operands are both
        upsampled.  Part of verify(): enable() plans again without them."""
        bad = {}
        for v in self.tracer.produced:
            m = v.producer
            if v.kind != "upsample" or m not in self.topdown_ups:
                continue
            for (c, pos) in v.consumers:
                ops = self.operands.get(c)
                other = ops[1 - pos] if ops is not None and pos < 2 else None
                if c not in self.add_resident or c not in self.plans or not self.plans[c].resident_add or other is None:
                    bad[m] = "the NewAdd %s that reads it is not resident (its other operand has no integer form)" % self._name(c)
                elif other.kind == "upsample" and (other.producer in self.topdown_ups or other is v):
                    bad[m] = "both operands of the NewAdd %s are upsampled" % self._name(c)
                elif other.shape is None or tuple(other.shape) != tuple(v.shape):
                    bad[m] = "the operands of the NewAdd %s differ in shape" % self._name(c)
        return bad

    def count_topdown(self):
        for v in self.tracer.produced:
            if v.kind == "add" and v.producer in self.topdown_adds and v.producer in self.plans:
                self.summary["topdown_adds"] += 1
                ups = [o.producer for o in self.operands[v.producer] if o.kind == "upsample" and o.producer in self.topdown_ups]
                self.summary["topdown_sum_sources"] += sum(1 for u in ups if self.topdown_ups[u][0] == 2)

    def _plan_avgpool_window(self, v):
        """`avgpool=True` plans a windowed nn.AvgPool2d (the pool branch of an Inception block, the 2x2 pool of a transition) that
        reads an int8 activation on a grid g and is read by NewConv2d layers only, all at one input bit b: DeQuantity -> pool ->
        the nn.ReLU behind it -> the consumers' Quantity run as one kernel on the integers (fq_avgpool_i8_nhwc), so the pool's
        source no longer has to leave as fp32 for it.  Its value has no exact integer form and gets NO entry in fmt: no Concat,
        add, max-pool, upsampling or second pool takes it as an operand, it is handed to those convolutions only.  Left in fp32
        form (out of scope): a NewAdd sum (int16) as the source, consumers that are not all convolutions at one bit, ceil_mode,
        divisor_override, windows above 64 taps, |bit - grid| > 8, a pool called twice; F.avg_pool2d and nn.AdaptiveAvgPool2d stay
        foreign.  The whole-plane pool in front of the head is served as before.  The summary then gains `resident_avgpools`.
        `avgpool=True, sums=True` lifts the first exclusion: a source whose format is (2, g), the exact int16 sum of a resident
        NewAdd -- the ResNet-D shortcut, AvgPool2d(2, 2) -> 1x1 convolution reading ReLU(sum) -- is taken under the same
        conditions and runs on fq_avgpool_i16_nhwc (the same rule; |S| <= 64 * 32768 < 2^24 keeps it exact).  The add then
        counts the pool as a reader of its exact integers (_readers) and writes no fp32 for it.  The pool's value still gets no
        entry in fmt.  A pool over a sum whose window happens to be the whole plane -- the last shortcut of a ResNet-D at a small
        input -- is planned the same way where its readers are convolutions (int8 out of one kernel instead of fp32 out of
        fq_avgpool_global_nhwc and a re-quantisation); where they are not (the head's pool in front of View) it keeps the
        whole-plane path.  The summary gains `resident_sum_avgpools`, and describe().avgpool_left names every hooked windowed
        pool that stays torch's with its reason."""
        m, e = v.producer, self.eff_of[id(v)][0]
        if self.avg_can_read(m):                            # the whole-plane pool: _AvgPoolResident ...
            f = self.fmt.get(id(v.src))
            if self.sw.sums and f is not None and f[0] == 2:    # ... unless it reads a sum and convolutions read it
                self._avgpool_window_declined(v, e)
            return None                                     # (the value itself has no integer format)
        why = self._avgpool_window_declined(v, e)
        if why is not None and self.sw.sums:
            self.left["avgpool_left"][m] = why
        return None

    def _avgpool_window_declined(self, v, e):
        """None when the windowed pool is planned (avg_resident), else why not."""
        m = v.producer
        f = self.fmt.get(id(v.src))
        if not self.once(m):
            return "the module was called more than once"
        if f is None:
            return "its source has no integer form in this plan (fp32 form)"
        if f[0] != 1 and not (self.sw.sums and f[0] == 2):
            return "its source is a NewAdd sum (int16): needs sums=True (fp32 form)"
        if m.ceil_mode:
            return "ceil_mode=True: only floor-mode pools are taken (fp32 form)"
        if not _avgpool_window_ok(m):
            return "divisor_override is set (fp32 form)"
        if e.foreign:
            return "read as fp32 by code outside the plan, or it is a model output"
        if not e.consumers:
            return "nothing reads it"
        for (c, _pos) in e.consumers:
            if not self.conv_can_read(c):
                return "read as fp32 by %s: only integer convolutions read a pooled value" % self._name(c)
        bits = set(c.input_bit for (c, _pos) in e.consumers)
        if len(bits) != 1:
            return "its readers quantise at different bits %s" % sorted(bits)
        b = bits.pop()
        k, st, pd = _pool_geometry(m)
        supported = _native.avgpool_i16_supported if f[0] == 2 else _native.avgpool_supported
        if min(st) < 1 or not supported(k, st, pd, b - f[1]):
            return ("window %dx%d, stride %s, padding %s, shift = bit %d - grid %d = %d: not taken by the kernel (at most 64 taps, "
                    "|shift| <= 8, 2 * padding <= kernel)" % (k[0], k[1], st, pd, b, f[1], b - f[1]))
        self.avg_resident[m] = (f[1], b)
        if f[0] == 2:
            self.avg_sum.add(m)
        return None

    def _integer_operands(self, m):
        """(value, value, format, format) of the two operands of a NewAdd / Concat called once, if both are integers; or None."""
        ops = self.operands.get(m)
        if not self.once(m) or ops is None or ops[0] is None or ops[1] is None:
            return None
        fx, fy = self.fmt.get(id(ops[0])), self.fmt.get(id(ops[1]))
        return (ops[0], ops[1], fx, fy) if fx is not None and fy is not None else None

    def _concat_format(self, v):
        """`concat=True` plans the Concat marker layer and nearest upsampling (nn.UpsamplingNearest2d, nn.Upsample(mode="nearest"))
        by an integer scale_factor of 2 or 4, both served by fq_concat_i8_nhwc: a Concat whose two operands are int8 activations
        on ONE grid -- what the calibrator's merge group gives them -- joins the integers, with the nn.ReLU behind it fused.
        Without the argument both are foreign code and their operands leave as fp32.  Left in fp32 form (out of scope): a Concat
        with a NewAdd sum (int16) as an operand or with operands on different grids, any dim but 1, more than two operands (nested
        Concats are flattened by defer_concats, `flatten=True`), the `size=` form and other factors of an upsampling; a bare torch.cat stays foreign, as a bare
        `+` does.  The summary then gains `resident_concats`, `resident_upsamples` and `fused_upsamples` (defer_upsamples)."""
        plain = self._concat_plain(v)
        if not self.sw.requant:
            return plain
        f, why = self._concat_requant(v, plain)
        if f is None and why is not None:
            self.left["requant_left"][v.producer] = why
        return f if f is not None else plain

    def _concat_plain(self, v):
        m = v.producer
        ops = self._integer_operands(m) if self.tracer.concat_ok.get(m) else None
        if ops is None:
            return None
        x, y, fx, fy = ops
        if fx[0] != 1 or fx != fy or x.shape is None or y.shape is None:
            return None
        if not _native.concat_supported([x.shape[1], y.shape[1]], [1, 1]):
            return None
        return fx

    def _concat_requant(self, v, plain):
        """`concat=True, requant=True` plans a Concat whose operands lie on grids g_i of their own and whose readers all quantise
        at one bit b on fq_concat_rq_i8_nhwc: the reference never re-quantises a Concat, so its chain DeQuantity_g_i -> cat ->
        (ReLU) -> Quantity_b is a closed integer function, r = rint(v * 2^(b - g_i)) clamped (include/fq.h).  An operand is an
        int8 activation ((1, g_i), directly or through a planned nearest upsampling, which defer_upsamples folds in), the exact
        int16 sum of a resident NewAdd ((2, g_i), with that add's fused ReLU; the add counts the Concat as a reader of its exact
        integers, _readers), or a lossy int8 value -- a table activation, a bilinear upsampling, another such Concat -- at bit b
        exactly.  The output is Quantity_b(cat(...)), a lossy value: planned with format (1, b) only where every transitive reader
        through _MOVES is an integer convolution at b (_lossy_walk) and |b - g_i| <= 8; verify() takes it back where
        a later pass left a reader in fp32 form.  The plain rule keeps every Concat it fully serves (operands int8 on one grid g,
        every convolution that reads it directly at g; a mover behind it takes its int8 as it is): this rule takes what that one
        refuses, or plans but has to emit fp32 for.  Returns (format, None) when planned, (None, why) when declined --
        describe().requant_left -- and (None, None) where the plain rule serves it."""
        m = v.producer
        direct = [c.input_bit for (c, _pos) in self.effective(v)[0].consumers if self.conv_can_read(c)]
        if plain is not None and all(bit == plain[1] for bit in direct):
            return None, None                               # (a mover behind it -- an outer Concat -- takes its int8 as it is)
        bits, fp32_reader = self._lossy_walk(v)
        ops = self.operands.get(m)
        if not self.once(m):
            return None, "the module was called more than once"
        if not self.tracer.concat_ok.get(m):
            return None, "dim != 1, or its operands are not two 4-D tensors"
        if ops is None or ops[0] is None or ops[1] is None:
            return None, "an operand is not the output of a planned layer (no integer source)"
        if m in self.revoked:
            return None, self.revoked[m]
        if fp32_reader is not None:
            return None, fp32_reader
        if len(bits) != 1:
            return None, "its readers quantise at different bits %s" % sorted(bits)
        b = next(iter(bits))
        fmts = []
        for o in ops:
            f = self.fmt.get(id(o))
            if f is None:
                src = self.fmt.get(id(o.src)) if o.kind == "upsample" and o.src is not None else None
                if src is not None and src[0] == 2:
                    return None, "an operand is an upsampled NewAdd sum: no integer kernel upsamples int16 (fp32 form)"
                return None, "an operand has no integer form in this plan (fp32 form)"
            root = o.src if o.kind == "relu" and o.src is not None else o
            if f[0] == 2 and root.kind != "add":
                return None, "an operand is int16 but no NewAdd sum (fp32 form)"
            if o.shape is None or len(o.shape) != 4:
                return None, "an operand is not 4-D"
            # (a lossy operand -- a table activation, a bilinear upsampling, another such Concat -- sits at b: its own walk went
            #  through this Concat to the same readers; the run-time path checks it all the same)
            if abs(b - f[1]) > 8:
                return None, "|b - g| = |%d - %d| > 8: not taken by the kernel (fp32 form)" % (b, f[1])
            fmts.append(f)
        if not _native.concat_rq_supported([o.shape[1] for o in ops], [1, 1], [f[0] for f in fmts], [b - f[1] for f in fmts]):
            return None, "fq_concat_rq_i8_nhwc does not take operands of %s channels (unsupported geometry)" % [o.shape[1] for o in ops]
        self.rq_cats.add(m)
        self.lossy[m] = b                                   # (also the plan's narrow_bit: the value's format)
        self.fields[m] = {"grid": tuple(f[1] for f in fmts)}
        self.forward_of[m] = _ConcatRequant
        self.summary["requant_concats"] += 1
        self.summary["requant_sum_sources"] += sum(1 for f in fmts if f[0] == 2)
        return (1, b), None

    def _shuffle_format(self, v):
        """`shuffle=True` plans nn.ChannelShuffle and the Slice marker (fabu_layer.Slice, x[:, start:stop]), both served by
        fq_shuffle_i8_nhwc: a module called once that reads a 4-D int8 activation permutes / copies the integers and hands them on
        the source's grid; its readers may be convolutions (dense, depthwise, grouped), a Concat, a max-pool, a windowed average
        pool, another shuffle or slice, or fp32 code.  No ReLU is fused into it (effective): a ReLU behind one reads the fp32
        form, as behind a max-pool.  Without the argument both are foreign code and their source leaves as fp32.  Left in fp32
        form (out of scope), each named with its reason by describe(): a NewAdd sum (int16) as the source, a module called twice,
        `start` / `stop` that are not plain ints with 0 <= start < stop <= C, groups that do not divide C, a non-4-D input, the
        call with nothing to do (Slice(0, C) of a C-channel source, one group); a Slice has no step and no axis but 1, and a bare
        chunk, split, slicing or torch.channel_shuffle call stays foreign, as a bare `+` does.  The summary then gains
        `resident_shuffles` and `resident_slices`."""
        m = v.producer
        src = self.fmt.get(id(v.src))
        why = None
        if not self.once(m):
            why = "the module was called more than once"
        elif src is None:
            why = "its source has no integer form in this plan (fp32 form)"
        elif src[0] != 1:
            why = "its source is a NewAdd sum (int16): only int8 activations are permuted (fp32 form)"
        elif v.src.shape is None or len(v.src.shape) != 4:
            why = "its input is not 4-D"
        else:
            channels = int(v.src.shape[1])
            geo = _shuffle_geometry(m, channels)
            if geo is None:
                why = ("groups = %r does not divide the %d channels" % (m.groups, channels) if v.kind == "shuffle" else
                       "start = %r, stop = %r are not plain ints with 0 <= start < stop <= %d" % (m.start, m.stop, channels))
            elif not _native.shuffle_supported(channels, *geo):
                why = "fq_shuffle_i8_nhwc does not take (c_off, C, groups) = %r of %d channels (nothing to do, or C > 65536)" % (
                    geo, channels)
            else:
                self.fields[m] = {"perm": geo}
                return src
        self.left["shuffle_left"][m] = why
        return None

    def _pixelshuffle_format(self, v):
        """`pixelshuffle=True` plans nn.PixelShuffle(r) and nn.PixelUnshuffle(r) -- the upsampler of a sub-pixel super-resolution
        network, the samplers of a restoration network, YOLOv2's passthrough -- on fq_pixel_shuffle_i8_nhwc: a module called once
        that reads a 4-D int8 activation (format (1, g), lossy or not) moves the integers between depth and space and hands them on
        the source's grid.  Both are pure permutations, so Quantity_b commutes with them: the kind is one of _MOVES and a lossy
        value walks through it.  Its readers are whatever a channel shuffle's may be: convolutions (dense, depthwise, grouped), a
        Concat (plain, flattened, re-quantising), a NewAdd, a max-pool, a windowed pool, a shuffle or slice, another pixel shuffle,
        or fp32 code and model outputs through to_f32().  No ReLU is fused into it (effective): a ReLU directly behind one reads the
        fp32 form; the common order, convolution + ReLU then pixel shuffle, fuses in the convolution as always.  Without the
        argument both modules are foreign code and their source leaves as fp32.  Plan.up carries the factor, Plan.perm the
        direction and the shallow tensor's channels.  Left to torch, each named with its reason by describe().pixelshuffle_left: a
        NewAdd sum (int16) as the source, a source without an integer form, a module called twice, a non-4-D input, a factor
        outside {2, 3, 4}, a geometry the kernel refuses; an F.pixel_shuffle call stays foreign, as a bare `+` does.  The summary
        gains `resident_pixelshuffles` and `resident_pixelunshuffles`."""
        m = v.producer
        src = self.fmt.get(id(v.src))
        why = None
        r = _pixel_factor(m)
        if not self.once(m):
            why = "the module was called more than once"
        elif v.src.shape is None or len(v.src.shape) != 4:
            why = "its input is not 4-D"
        elif src is None:
            why = "its source has no integer form in this plan (fp32 form)"
        elif src[0] != 1:
            why = "its source is a NewAdd sum (int16): only int8 activations are permuted (fp32 form)"
        elif type(r) is not int or r not in PIXEL_FACTORS:
            why = "factor %r: only the factors 2, 3 and 4 are taken (fp32 form)" % (r,)
        else:
            geo = _pixel_geometry(m, v.src.shape)
            if geo is None or not _native.pixel_shuffle_supported(geo[1][1], geo[0], geo[1][0] == "s2d"):
                why = "fq_pixel_shuffle_i8_nhwc does not take r = %d on an input of shape %s (unsupported geometry)" % (r, tuple(v.src.shape))
            else:
                self.fields[m] = {"up": geo[0], "perm": geo[1]}
                return src
        self.left["pixelshuffle_left"][m] = why
        return None

    def _name(self, m):
        return self.names.get(m) or type(m).__name__

    def _act_format(self, v):
        """`activations=True` plans the elementwise activations of ACTIVATION_TYPES (nn.LeakyReLU, nn.PReLU with one weight,
        nn.Hardswish, nn.Hardsigmoid, nn.SiLU, nn.Sigmoid, nn.Tanh, nn.ELU, nn.Hardtanh, nn.Mish, nn.GELU) on fq_act_lut_i8_nhwc:
        between an int8 activation q on grid g and convolutions that quantise at bit b, f is the table
        T[q + 128] = Quantity_b(f(DeQuantity_g(q))), built at enable() time with the library's own ops and the module's own
        forward (_native.build_act_table) and kept on the module's plan -- changing an nn.PReLU weight afterwards needs a new
        enable().  The table's output is Quantity_b(f(x)), not f(x) (the lossy-value rule): it is planned as an
        int8 value on grid b only where every transitive reader -- through max-pools, Concats, nearest upsamplings, shuffles
        and slices, with which Quantity_b commutes -- is an integer convolution with input_bit == b (_lossy_walk), and
        verify() takes it back where a later pass left one of those readers in fp32 form.  Left to torch, each named with
        its reason by describe().activations_left: a module called twice, a NewAdd sum (int16) as the source, a non-4-D input, a
        per-channel nn.PReLU, a source without an integer form, readers at two bits, any fp32 reader (an average pool, a NewAdd, a
        second table activation, a model output, foreign code), and `inplace=True` modules: the planned forward returns a new
        activation and cannot rewrite the tensor that other readers may hold by its earlier name.  The summary then gains
        `resident_activations`."""
        m = v.producer
        src = self.fmt.get(id(v.src))
        why = None
        if not self.once(m):
            why = "the module was called more than once"
        elif m in self.tracer.inplace or getattr(m, "inplace", False):
            why = "inplace=True: the module rewrites its input tensor, a table activation returns a new one (fp32 form)"
        elif isinstance(m, nn.PReLU) and m.num_parameters != 1:
            why = "a per-channel nn.PReLU (%d weights) is no function of the integer alone" % m.num_parameters
        elif v.src.shape is None or len(v.src.shape) != 4:
            why = "its input is not 4-D"
        elif src is None:
            why = "its source has no integer form in this plan (fp32 form)"
        elif src[0] != 1:
            why = "its source is a NewAdd sum (int16): only int8 activations go through the table (fp32 form)"
        elif not _native.act_lut_supported(int(v.src.shape[1])):
            why = "fq_act_lut_i8_nhwc does not take %d channels" % int(v.src.shape[1])
        elif m in self.revoked:
            why = self.revoked[m]
        else:
            bits, why = self._lossy_walk(v)
            if why is None and len(bits) != 1:
                why = "its readers quantise at different bits %s" % sorted(bits)
            if why is None:
                self.lossy[m] = bits.pop()
                self.fields[m] = {"grid": src[1]}
                return (1, self.lossy[m])
        self.left["activations_left"][m] = why
        return None

    def _bilinear_format(self, v):
        """`concat=True, bilinear=True` plans nn.Upsample(scale_factor=2 or 4, mode="bilinear", align_corners=False) -- the decoder
        step of a U-Net, DeepLabV3+ or BiSeNet -- on fq_upsample_bilinear_i8_nhwc: between an int8 activation q on grid g and
        convolutions that quantise at bit b the chain DeQuantity_g -> interpolation -> (ReLU) -> Quantity_b is a closed integer
        function (weights are odd multiples of 1 / (2 up): one rounding of S * 2^(b - g) / (2 up)^2, include/fq.h).  Its output is
        Quantity_b(up(x)), not up(x): the lossy-value rule of _act_format applies word for word -- planned as an int8 value on grid
        b only where every transitive reader through _MOVES is an integer convolution with input_bit == b (_lossy_walk), taken
        back by verify() where a later pass left one of those readers in fp32 form.  The kind is NOT one of _MOVES:
        Quantity_b does not commute with interpolation, so a table activation (or another bilinear upsampling) in front of one
        is left by _lossy_walk.  An nn.ReLU directly behind the module is the kernel's `relu` flag (effective, _take).  Left to
        torch, each named with its reason by describe().bilinear_left: align_corners=True, the `size=` form, another or a
        non-integer factor, a module called twice, a NewAdd sum (int16) as the source, a lossy source, a source without an integer
        form, readers at two bits, any fp32 reader (a NewAdd, an average pool, a table activation, a model output, foreign code),
        |b - g| > 8.  The summary then gains `resident_bilinears`."""
        m = v.producer
        src = self.fmt.get(id(v.src))
        why = _bilinear_form_left(m)
        if why is not None:
            pass
        elif not self.once(m):
            why = "the module was called more than once"
        elif v.src.shape is None or len(v.src.shape) != 4:
            why = "its input is not 4-D"
        elif self._lossy_origin(v.src) is not None:
            why = ("its source is the lossy value of %s: Quantity_b does not commute with interpolation, so that module stays torch's "
                   "and this one reads fp32" % self._name(self._lossy_origin(v.src)))
        elif src is None:
            why = "its source has no integer form in this plan (fp32 form)"
        elif src[0] != 1:
            why = "its source is a NewAdd sum (int16): only int8 activations are interpolated (fp32 form)"
        elif m in self.revoked:
            why = self.revoked[m]
        else:
            bits, why = self._lossy_walk(v)
            if why is None and len(bits) != 1:
                why = "its readers quantise at different bits %s" % sorted(bits)
            if why is None:
                b = bits.pop()
                if not _native.upsample_bilinear_supported(_bilinear_factor(m), b - src[1]):
                    why = "|b - g| = |%d - %d| > 8: not taken by the kernel (fp32 form)" % (b, src[1])
                else:
                    self.lossy[m] = b
                    self.fields[m] = {"up": _bilinear_factor(m), "grid": src[1]}
                    return (1, b)
        self.left["bilinear_left"][m] = why
        return None

    def _lossy_origin(self, v, depth=0):
        """The table activation, bilinear upsampling or (planned) re-quantising Concat whose (would-be) lossy value reaches v
        through ReLUs and _MOVES, or None.  Decided on the trace and on what was planned in front of v."""
        if v is None or depth > 64:
            return None
        if v.kind in ("act", "bilinear"):
            return v.producer
        if v.kind == "concat":
            if v.producer in self.rq_cats:                  # (a re-quantising Concat: its own value is Quantity_b(cat(...)))
                return v.producer
            for o in self.operands.get(v.producer) or ():
                found = self._lossy_origin(o, depth + 1)
                if found is not None:
                    return found
            return None
        if v.kind == "relu" or v.kind in _MOVES:
            return self._lossy_origin(v.src, depth + 1)
        return None

    def _lossy_walk(self, v):
        """({input bits of the convolutions that read v, directly or through _MOVES}, None), or (_, why not): the first reader
        that would see the value in fp32 form.  Decided on the trace alone, before the movement modules are planned."""
        bits = set()
        e, _relu = self.effective(v)
        if e.foreign or v.foreign:
            return bits, "read as fp32 by code outside the plan, or it is a model output"
        if not e.consumers:
            return bits, "nothing reads it"
        for (c, _pos) in e.consumers:
            if self.conv_can_read(c):
                bits.add(c.input_bit)
                continue
            nxt = self.value_of.get(c)
            if nxt is not None and nxt.kind in _MOVES and self.once(c):
                more, why = self._lossy_walk(nxt)
                if why is not None:
                    return bits, why
                bits |= more
                continue
            what = {"add": "the NewAdd", "avgpool": "the average pool", "act": "the table activation", "relu": "the ReLU",
                    "bilinear": "the bilinear upsampling"}.get(
                self.tracer._kind(c) if not isinstance(c, nn.AvgPool2d) else "avgpool", "the module")
            return bits, "read as fp32 by %s %s" % (what, self._name(c))
        return bits, None

    def verify(self):
        """{module: why} for every planned lossy producer -- table activation, bilinear upsampling, re-quantising Concat -- whose
        value, after all passes, somebody would read in fp32 form: a producer on the way that emits fp32, or a reader that turned
        out unplanned (a Concat whose other operand sits on another grid); and for the upsamplings that verify_topdown() names.
        enable() plans again without them: the module stays torch's (a Concat keeps the plain rule's plan) and its source leaves
        as fp32, as without the switch.  At most one round per module."""
        bad = {}
        for m, b in self.lossy.items():
            why = self._lossy_violation(self.value_of[m], b)
            if why is not None:
                bad[m] = "revoked by the lossy rule: " + why
        bad.update(self.verify_topdown())
        return bad

    def _lossy_violation(self, v, b):
        e = self.eff_of[id(v)][0]
        for (c, _pos) in e.consumers:
            if self.conv_can_read(c) and c.input_bit == b:
                continue
            nxt = self.value_of.get(c)
            if c in self.int8_resident and c in self.plans and nxt is not None and nxt.kind in _MOVES:
                why = self._lossy_violation(nxt, b)
                if why is not None:
                    return why
                continue
            return "read as fp32 by %s" % self._name(c)
        plan = self.plans.get(v.producer)
        if plan is None or plan.emit_f32 or e.foreign:
            return "read as fp32 behind %s" % self._name(v.producer)
        return None

    def _add_format(self, v):
        """A NewAdd of two integer operands: the exact sum as int16 on the finer of their grids, where that fits."""
        m = v.producer
        ops = self._integer_operands(m)
        if ops is None:
            return None
        gx, gy = ops[2][1], ops[3][1]
        g = max(0, gx, gy)
        if g > MAX_WIDE_GRID or min(gx, gy) < -16:
            return None
        self.add_resident.add(m)
        if any(o.kind == "upsample" and o.producer in self.topdown_ups for o in ops[:2]):
            self.topdown_adds.add(m)
        return (2, g)

    # ---- pass 2: what every producer has to emit

    def plan_outputs(self):
        for v in self.tracer.produced:
            e, relu_mod = self.eff_of[id(v)]
            if v.kind == "avgpool":
                if v.producer in self.avg_resident:
                    plan = Plan()
                    plan.emit_int, plan.emit_f32 = True, False
                    plan.grid, plan.narrow_bit = self.avg_resident[v.producer]
                    self._take(v.producer, plan, relu_mod, _KIND[v.kind].forward)
                    self.summary[_KIND[v.kind].counter] += 1
                    if v.producer in self.avg_sum:
                        self.summary["resident_sum_avgpools"] += 1
            elif id(e) in self.fmt:                         # (anything else stays a plain fp32 producer)
                self._plan_output(v, e, relu_mod)

    def _take(self, m, plan, relu_mod, forward=None):
        """Module m emits what `plan` says, with the nn.ReLU behind it (if any) fused and, for a module that is no integer
        layer itself, `forward` as its instance-level forward."""
        plan.relu = relu_mod is not None
        plan.clip = isinstance(relu_mod, nn.ReLU6)
        self.plans[m] = plan
        if plan.relu:
            self.forwards.append((relu_mod, _ReluPassThrough(relu_mod)))
            self.summary["fused_relu6s" if plan.clip else "fused_relus"] += 1
        if forward is not None:
            self.forwards.append((m, forward(m)))
        self.summary["fp32_outputs" if plan.emit_f32 else "int_only_outputs"] += 1

    def _readers(self, v, e):
        """Who reads the value: (somebody needs the fp32 tensor, readers of the exact integers, other readers of the int8 form,
        [the input bit of every convolution that reads it])."""
        need_f32, exact, int8, bits = e.foreign, 0, 0, []
        for (c, _pos) in e.consumers:
            if self.conv_can_read(c):
                bits.append(c.input_bit)
            elif (c in self.add_resident or self.avg_can_read(c) or (v.kind == "add" and c in self.avg_sum)
                  or (v.kind == "add" and c in self.topdown_ups) or (v.kind == "add" and c in self.rq_cats)):
                exact += 1                                  # (a windowed pool over the sum reads the exact int16, as the whole-plane pool does;
                                                            #  so does an upsampling in front of a NewAdd, topdown=True, and a
                                                            #  re-quantising Concat, requant=True)
            elif (c in self.int8_resident or c in self.avg_resident) and v.kind != "add":
                int8 += 1                                   # int8 max-pool / Concat / nearest upsampling / windowed average pool
            else:
                need_f32 = True
        return need_f32, exact, int8, bits

    def _plan_output(self, v, e, relu_mod):
        m = v.producer
        plan = Plan()
        need_f32, exact, int8, bits = self._readers(v, e)
        plan.want_wide = exact > 0
        if v.kind == "add":
            plan.resident_add = True
            plan.grid = self.fmt[id(e)][1]
            plan.narrow_bit = bits[0] if bits else None
        else:
            plan.narrow_bit = self.fmt[id(e)][1]            # (a convolution's own output bit)
        served = bits.count(plan.narrow_bit)
        if served != len(bits):
            need_f32 = True                                 # a consumer quantises at another bit: from fp32
        if v.kind == "add" and need_f32:
            plan.want_wide = True                           # fp32 leaves through the exact int16 sum
        plan.emit_int = exact + int8 + served > 0
        plan.emit_f32 = need_f32 or not plan.emit_int
        for field, value in self.fields.get(m, {}).items():    # (what the format rule decided for this module)
            setattr(plan, field, value)
        row = _KIND[v.kind]
        self._take(m, plan, relu_mod, self.forward_of.get(m, row.forward))
        self.summary[row.counter(m) if callable(row.counter) else row.counter] += 1

    # ---- fusion passes (in this order: fuse_projections reads the fuse_next that fuse_block_tails sets)

    def defer_convs(self):
        """A convolution whose value goes to one resident add and nowhere else is run BY that add (DeferredConv)."""
        self.summary["fused_conv_adds"] = 0
        for add_mod, add_plan, ops, _va in self.resident_adds():
            if add_mod in self.topdown_adds:                # (its other operand stays a handle: the lateral convolution launches itself)
                continue
            for pos in (0, 1):
                v = ops[pos]
                plan = self.plans.get(v.producer) if isinstance(v.producer, self.conv_type) else None
                if (v.kind == "contraction" and plan is not None and not plan.depthwise and not plan.grouped and not plan.relu
                        and not plan.emit_f32 and not v.foreign and v.consumers == [(add_mod, pos)] and ops[1 - pos] is not v
                        and not add_plan.emit_f32):
                    plan.defer = True
                    add_plan.fuse_arg = pos
                    self.summary["fused_conv_adds"] += 1
                    break

    def fuse_block_tails(self):
        """When the re-quantised sum of an add that runs its conv3 feeds a 1x1 convolution (the next bottleneck's conv1), that
        convolution runs inside the same kernel (fq_block_tail_i8, Plan.fuse_next): its operand is staged in LDS and, if nobody
        else reads it, never written."""
        self.summary["fused_block_tails"] = 0
        for _add_mod, plan, ops, va in self.resident_adds():
            if plan.fuse_arg is None or plan.emit_f32 or not plan.want_wide or not block_tail_enabled():
                continue
            conv3 = ops[plan.fuse_arg].producer
            other = self.fmt.get(id(ops[1 - plan.fuse_arg]))                     # (bytes, grid) of the shortcut
            if other is None or not _pointwise_conv(conv3.Conv):
                continue
            readers = [c for (c, _pos) in self.eff_of[id(va)][0].consumers if self.conv_can_read(c)]
            for c in readers:
                cp = self.plans.get(c)
                # (not cp.clip: the second tail of fq_block_tail_i8 has the plain ReLU's range only; a 1x1 with a fused ReLU6
                #  stays a launch of its own)
                if (cp is not None and not cp.defer and not cp.grouped and not cp.clip and cp.emit_int and not cp.emit_f32
                        and self.once(c) and isinstance(c, self.conv_type)
                        and _pointwise_conv(c.Conv) and c.input_bit == plan.narrow_bit
                        and conv3.Conv.out_channels == c.Conv.in_channels
                        and _native.block_tail_supported(conv3.Conv.in_channels, conv3.Conv.out_channels, c.Conv.out_channels,
                                                         conv3._rs(), c._rs(), conv3.output_bit, other[1], other[0],
                                                         plan.narrow_bit)):
                    plan.fuse_next = c
                    plan.narrow_to_hbm = len(readers) > 1
                    self.summary["fused_block_tails"] += 1
                    break

    def fuse_projections(self):
        """When the OTHER operand of such an add is a 1x1 projection of the block's input that nobody else reads (the first block
        of a stage), the kernel computes that convolution as well (fq_block_tail_proj_i8, Plan.fuse_proj): its K3 bytes per pixel
        are neither written nor read back."""
        self.summary["fused_projections"] = 0
        for add_mod, plan, ops, _va in self.resident_adds():
            if plan.fuse_arg is None or plan.emit_f32 or not block_tail_enabled() or not block_tail_proj_enabled():
                continue
            conv3, vp = ops[plan.fuse_arg].producer, ops[1 - plan.fuse_arg]
            proj = vp.producer
            pp = self.plans.get(proj) if isinstance(proj, self.conv_type) else None
            if (vp.kind != "contraction" or pp is None or pp.relu or pp.emit_f32 or pp.defer or pp.grouped or vp.foreign
                    or vp.consumers != [(add_mod, 1 - plan.fuse_arg)] or not self.conv_can_read(proj) or not self.once(proj)):
                continue
            k3, kp = conv3.Conv, proj.Conv
            nxt = plan.fuse_next
            if (not _pointwise_conv(kp, any_stride=True) or not _pointwise_conv(k3)
                    or kp.out_channels != k3.out_channels or (kp.out_channels % 16) or (kp.in_channels % 16)
                    or not _native.block_tail_proj_supported(k3.in_channels, k3.out_channels,
                                                             nxt.Conv.out_channels if nxt is not None else 0, kp.in_channels,
                                                             conv3._rs(), nxt._rs() if nxt is not None else 0, proj._rs(),
                                                             kp.stride[0])):
                continue
            pp.defer = True
            plan.fuse_proj = True
            self.summary["fused_projections"] += 1

    def defer_upsamples(self):
        """(`concat=True`) A nearest upsampling whose value goes to one resident Concat and nowhere else is not launched at all:
        the Concat reads the small tensor with the factor as its operand's `up` (DeferredUpsample)."""
        self.summary["fused_upsamples"] = 0
        for v in self.tracer.produced:
            plan = self.plans.get(v.producer)
            if (v.kind != "upsample" or plan is None or plan.up is None or plan.relu or plan.emit_f32 or v.foreign
                    or v.producer in self.topdown_ups):
                continue
            if (len(v.consumers) != 1 or v.consumers[0][0] not in self.int8_resident
                    or not isinstance(v.consumers[0][0], self.concat_type)):
                continue
            cat_mod, pos = v.consumers[0]
            ops = self.operands[cat_mod]
            ups = [1, 1]
            ups[pos] = plan.up
            if ops[pos] is not v or ops[1 - pos] is v or not _native.concat_supported([ops[0].shape[1], ops[1].shape[1]], ups):
                continue
            plan.defer = True
            self.summary["fused_upsamples"] += 1

    def defer_concats(self):
        """(`concat=True, flatten=True`) A resident Concat whose value -- behind its own fused nn.ReLU, if it has one -- goes to one
        operand of one other resident Concat and nowhere else is not launched: the consumer takes its leaves into its own source
        list and launches once (DeferredConcat, fq_concat_n_i8_nhwc), the inner ReLU as those leaves' flag.  Values are walked
        in traced order, so an inner Concat's leaf count is final when its consumer is looked at.  A Concat that would push its
        consumer past MAX_CONCAT_LEAVES is not deferred and launches on its own; an upsampling between two Concats ends the
        flattening (the inner one launches, the upsampling is still folded into the outer one).  Left out: NewAdd sums as
        operands, more than eight leaves per launch, factor products through nested upsamplings, a bare torch.cat.  The
        summary gains `flattened_concats`; `resident_concats` keeps counting planned markers."""
        cat_of = dict((id(self.eff_of[id(v)][0]), v) for v in self.tracer.produced if v.kind == "concat")
        leaves = {}                      # id(Concat value) -> sources of its launch

        def count(cat_mod, assume=None):
            n = 0
            for op in self.operands[cat_mod]:
                inner = cat_of.get(id(op))
                plan = self.plans.get(inner.producer) if inner is not None else None
                n += leaves[id(inner)] if inner is not None and (inner is assume or (plan is not None and plan.defer)) else 1
            return n

        for v in self.tracer.produced:
            plan = self.plans.get(v.producer)
            if v.kind != "concat" or plan is None or v.producer not in self.int8_resident:
                continue
            leaves[id(v)] = count(v.producer)
            if v.producer in self.rq_cats:                  # (a re-quantising Concat launches itself: its leaves are on other grids)
                continue
            e = self.eff_of[id(v)][0]
            if v.foreign or e.foreign or plan.emit_f32 or len(e.consumers) != 1:
                continue
            cat_mod, pos = e.consumers[0]
            if (not isinstance(cat_mod, self.concat_type) or cat_mod not in self.int8_resident or cat_mod not in self.plans
                    or pos > 1 or cat_mod in self.rq_cats):     # (... and takes an inner plain Concat as ONE int8 source)
                continue
            ops = self.operands[cat_mod]
            if ops[pos] is not e or ops[1 - pos] is e or count(cat_mod, assume=v) > MAX_CONCAT_LEAVES:
                continue
            plan.defer = True
            self.summary["flattened_concats"] += 1

    def hook_global_pools(self):
        for m in self.tracer.avgpool_shapes:
            if self.avg_can_read(m) and m not in self.avg_resident:
                self.forwards.append((m, _AvgPoolResident(m)))
                self.summary["resident_pools"] += 1

    def install(self, model):
        for m, plan in self.plans.items():
            m.__dict__["_resident"] = plan
        for m, forward in self.forwards:
            m.__dict__["forward"] = forward
        model.__dict__["_fq_resident_enabled"] = True
        names = dict((m, name) for name, m in model.named_modules())
        report = model.__dict__["_fq_resident_report"] = {}      # what describe() hands out besides the plans: attribute -> value
        for row in _KINDS:                                  # a hooked module that ran and has neither a plan nor a reason yet
            if row.default is not None and getattr(self.sw, row.switch):
                for m in self.tracer.seen[row.report]:
                    if m not in self.plans and m not in self.left[row.report]:
                        self.left[row.report][m] = row.default(m) if callable(row.default) else row.default
        if self.sw.relu6:
            self._relu6_reasons()
            report["fused_relu6s"] = self.summary["fused_relu6s"]
        if self.sw.deconv:
            self._deconv_reasons()
        if self.sw.sums:
            self._unplanned_avgpools()
        if self.sw.topdown:
            self._foreign_upsamples(model)
        if self.sw.activations:
            for m, plan in self.plans.items():
                if _is_table_activation(m):
                    plan.table = _native.build_act_table(m, plan.grid, plan.narrow_bit)
            report["activations_revoked"] = tuple(names.get(m, "?") for m in self.revoked if _is_table_activation(m))
        for switch, _keys, attributes in _SWITCH_TABLE:
            for attribute in attributes if getattr(self.sw, switch) else ():
                report[attribute] = dict((names.get(m, "?"), why) for m, why in self.left[attribute].items())

    def _unplanned_avgpools(self):
        """(`sums=True`) avgpool_left also names every hooked pool that ran without a plan, one behind foreign code included."""
        for m in self.tracer.calls:
            if (isinstance(m, nn.AvgPool2d) and m not in self.plans and m not in self.left["avgpool_left"]
                    and not self.avg_can_read(m)):
                self.left["avgpool_left"][m] = "its input is not the output of a planned layer (no integer source)"

    def _foreign_upsamples(self, model):
        """(`topdown=True`) topdown_left also names what _trace did not hook: foreign code."""
        for m in model.modules():
            if isinstance(m, nn.Upsample) and _upsample_factor(m) is None and m not in self.lossy:
                self.left["topdown_left"][m] = ("no nearest upsampling by one integer scale_factor of 2 or 4 (a `size=` form, another "
                                                "factor or another mode): foreign code")


def _named(*names):
    """Recognises the library's own layers by class name (new_quantity_op imports this module, so it is not imported up here)."""
    return lambda m: any(c.__name__ in names for c in type(m).__mro__)


def _instance_of(*types):
    return lambda m: isinstance(m, types)


def _pixel_counter(m):
    return "resident_pixelunshuffles" if isinstance(m, nn.PixelUnshuffle) else "resident_pixelshuffles"


_NO_SOURCE = "its input is not the output of a planned layer (no integer source)"
_Kind = collections.namedtuple("_Kind", "name match rule switch behind fuse_relu moves forward counter report default")
_Kind.__new__.__defaults__ = (None, False, True, False, None, None, None, None)      # (of `switch` ... `default`)
# One row per traced kind; the first row that matches a hooked module is its kind, the last row is what any other hooked module
# is.  Everything that tells kinds apart reads this table -- to add an op: a row, its format rule, its forward, its enable() switch.
#   name      : _Value.kind
#   match     : recognises the module
#   rule      : its format rule, rule(planning, value) -> (bytes, grid) or None (_Planning.plan_formats); the docstring of the rule
#               is the specification of its switch
#   switch    : the enable() switch that hooks it in _trace (None: always hooked; without its switch a module stays foreign code)
#   behind    : its value exists only behind a traced value (_Tracer.post)
#   fuse_relu : an nn.ReLU that is its only reader may be fused into it (_Planning.effective)
#   moves     : Quantity_b commutes with it -- data movement and max --, so a lossy value walks through it (_MOVES).  Not the
#               bilinear upsampling: Quantity_b does not commute with interpolation
#   forward   : its instance-level forward where planned (None: an integer layer, which reads its plan itself)
#   counter   : the summary key that counts the planned ones, or a function of the module that gives it
#   report    : the attribute of describe() that names the hooked ones that stay torch's (and the key of _Tracer.seen)
#   default   : the reason given to one that ran without a plan and without a reason of its own (a text, or a function of the
#               module; None: its report is written by a function of its own)
_KINDS = (
    _Kind("relu", _instance_of(nn.ReLU), None, behind=True),
    _Kind("relu", _instance_of(nn.ReLU6), None, "relu6", behind=True, report="relu6_left"),
    _Kind("maxpool", _instance_of(nn.MaxPool2d), _Planning._maxpool_format, behind=True, fuse_relu=False, moves=True,
          forward=_MaxPoolResident, counter="resident_pools"),
    _Kind("avgpool", _instance_of(nn.AvgPool2d), _Planning._plan_avgpool_window, behind=True, forward=_AvgPoolWindowResident,
          counter="resident_avgpools"),
    _Kind("bilinear", lambda m: isinstance(m, nn.Upsample) and m.mode == "bilinear", _Planning._bilinear_format, "bilinear",
          behind=True, forward=_BilinearResident, counter="resident_bilinears", report="bilinear_left",
          default=lambda m: _bilinear_form_left(m) or _NO_SOURCE),
    _Kind("upsample", lambda m: _upsample_factor(m) is not None, _Planning._upsample_format, "concat", behind=True, moves=True,
          forward=_UpsampleResident, counter="resident_upsamples"),
    _Kind("shuffle", _instance_of(nn.ChannelShuffle), _Planning._shuffle_format, "shuffle", behind=True, fuse_relu=False, moves=True,
          forward=_ShuffleResident, counter="resident_shuffles", report="shuffle_left",
          default="its input is not the output of a planned layer"),
    _Kind("act", _is_table_activation, _Planning._act_format, "activations", behind=True, fuse_relu=False,
          forward=_ActTableResident, counter="resident_activations", report="activations_left", default=_NO_SOURCE),
    _Kind("pixelshuffle", _instance_of(nn.PixelShuffle, nn.PixelUnshuffle), _Planning._pixelshuffle_format, "pixelshuffle",
          behind=True, fuse_relu=False, moves=True, forward=_PixelShuffleResident, counter=_pixel_counter,
          report="pixelshuffle_left", default=_NO_SOURCE),
    _Kind("concat", _named("Concat"), _Planning._concat_format, "concat", moves=True, forward=_ConcatResident,
          counter="resident_concats"),
    _Kind("add", _named("NewAdd"), _Planning._add_format, counter="resident_adds"),
    _Kind("slice", _named("Slice"), _Planning._shuffle_format, "shuffle", behind=True, fuse_relu=False, moves=True,
          forward=_SliceResident, counter="resident_slices", report="shuffle_left",
          default="its input is not the output of a planned layer"),
    _Kind("contraction", _named("NewConv2d", "NewLinear", "NewConvTranspose2d"), _Planning._conv_format, counter="resident_convs"),
)
_KIND = dict((row.name, row) for row in reversed(_KINDS))    # (by name; the two rows of "relu" differ in how they are hooked only)
_MOVES = tuple(row.name for row in _KINDS if row.moves)     # what Quantity_b commutes with: data movement and max


def _row(module):
    """The row of _KINDS that a hooked module belongs to."""
    for row in _KINDS:
        if row.match(module):
            return row
    return _KINDS[-1]


def _trace(model, example_input, switches):
    """One forward of `model` in eval mode under the tracer: (tracer, the outputs of that forward)."""
    tracer = _Tracer(switches.avgpool)
    hooks = []
    for m in model.modules():
        row = _row(m)
        if not row.match(m) or (row.switch is not None and not getattr(switches, row.switch)):
            continue                                        # (foreign code: no kind, or one whose switch is off)
        if row.name == "concat":                            # (`dim`, and the operands themselves, may be given by name)
            hooks.append(m.register_forward_pre_hook(tracer.pre_concat, with_kwargs=True))
        else:
            hooks.append(m.register_forward_pre_hook(tracer.pre))
        hooks.append(m.register_forward_hook(tracer.post))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            with tracer:
                traced_out = model(example_input)
            tracer.mark_foreign(traced_out)
    finally:
        for h in hooks:
            h.remove()
        model.train(was_training)
    return tracer, traced_out


def enable(model, example_input, verify=True, depthwise=False, concat=False, avgpool=False, grouped=False, relu6=False,
           flatten=False, shuffle=False, activations=False, sums=False, topdown=False, bilinear=False, requant=False,
           pixelshuffle=False, deconv=False):
    """Trace one forward of `model` (an integer-simulation model built by Reconstruction.ReconModel,
    on the GPU) and switch every eligible NewConv2d / NewAdd (and the nn.ReLU / nn.MaxPool2d / global
    nn.AvgPool2d between them) to resident integer activations.  Returns a summary dict.
    `example_input` is any valid input batch; the plan does not depend on its size.  With `verify`
    (default) the planned model is run once on `example_input` and must reproduce the traced forward
    bit for bit, otherwise the plan is removed and FqError raised.
    Opt-in, each adding its own keys to the summary and leaving the plan as it was when off:
    `depthwise=True` also plans depthwise NewConv2d layers (_Planning.is_dw), `grouped=True` grouped ones (_Planning.is_gc);
    `concat=True` also plans the Concat marker layer and nearest upsampling by 2 or 4 (_Planning._concat_format, defer_upsamples);
    `avgpool=True` also plans a windowed nn.AvgPool2d between an int8 activation and convolutions (_plan_avgpool_window);
    `relu6=True` also fuses an nn.ReLU6 behind a NewConv2d, as an nn.ReLU is fused (_Planning.takes_relu6);
    `flatten=True` (with `concat=True`; ValueError without) runs nested Concats as one launch (_Planning.defer_concats);
    `shuffle=True` also plans nn.ChannelShuffle and the Slice marker on the int8 integers (_Planning._shuffle_format);
    `activations=True` also plans elementwise activations that are no clamp (nn.LeakyReLU, nn.Hardswish, nn.SiLU, ...) as a
    256-entry table between integer layers (_Planning._act_format).  The tables are built here: changing an nn.PReLU weight
    afterwards needs a new enable();
    `sums=True` (with `avgpool=True`; ValueError without) lets such a windowed pool read the exact int16 sum of a NewAdd -- the
    ResNet-D shortcut -- on fq_avgpool_i16_nhwc (_plan_avgpool_window);
    `topdown=True` (with `concat=True`; ValueError without) lets a NewAdd read an operand through a nearest upsampling by 2 or 4
    -- the FPN top-down step, over an int8 activation or the int16 sum of the add above -- on fq_add_up_resident, the upsampled
    tensor never written (_Planning._topdown_format);
    `bilinear=True` (with `concat=True`; ValueError without) also plans nn.Upsample(scale_factor=2 or 4, mode="bilinear",
    align_corners=False) between an int8 activation and convolutions at one bit -- the decoder step of a U-Net -- on
    fq_upsample_bilinear_i8_nhwc, a lossy value like a table activation's (_Planning._bilinear_format);
    `requant=True` (with `concat=True`; ValueError without) also plans a Concat whose operands lie on different grids, whose
    readers quantise at another bit than its operands, or one of whose operands is the int16 sum of a NewAdd -- the skip of a
    ResNet-encoder U-Net -- on fq_concat_rq_i8_nhwc, which re-quantises every source to the readers' bit: a lossy value too
    (_Planning._concat_requant);
    `pixelshuffle=True` also plans nn.PixelShuffle(r) and nn.PixelUnshuffle(r), r in {2, 3, 4}, on the int8 integers
    (fq_pixel_shuffle_i8_nhwc; _Planning._pixelshuffle_format).  It needs no other switch;
    `deconv=True` also plans NewConvTranspose2d layers -- the learned upsampling of a U-Net, a pix2pix / DCGAN head, a LinkNet
    decoder -- as integer producers and consumers on fq_deconv2d_i8_resident (_Planning.is_dc).  It needs no other switch."""
    from .new_quantity_op import QUANTIZE_BIT
    switches = _switches(depthwise=depthwise, concat=concat, avgpool=avgpool, grouped=grouped, relu6=relu6, flatten=flatten,
                         shuffle=shuffle, activations=activations, sums=sums, topdown=topdown, bilinear=bilinear, requant=requant,
                         pixelshuffle=pixelshuffle, deconv=deconv)
    for switch, needed, message in _SWITCH_NEEDS:
        if getattr(switches, switch) and not getattr(switches, needed):
            raise ValueError(message)
    _clear(model)
    if QUANTIZE_BIT != 8:
        raise _native.FqError("resident activations are defined for QUANTIZE_BIT = 8")
    tracer, traced_out = _trace(model, example_input, switches)
    names = dict((m, name) for name, m in model.named_modules())
    revoked = {}
    while True:
        planning = _Planning(tracer, switches, revoked, names)
        planning.plan_formats()
        planning.plan_outputs()
        planning.defer_convs()
        planning.fuse_block_tails()
        planning.fuse_projections()
        if switches.concat:
            planning.defer_upsamples()
        if switches.flatten:
            planning.defer_concats()
        planning.hook_global_pools()
        bad = planning.verify()
        if not bad:
            break
        revoked.update(bad)                                 # (each round takes at least one module out -- a table activation, an
        #                                                      upsampling, a re-quantising Concat --: it ends)
    if switches.topdown:
        planning.count_topdown()
    planning.install(model)
    if verify:
        with torch.no_grad():
            planned_out = model(example_input)
        same = all(torch.equal(a, b) for a, b in zip(_iter_tensors(planned_out), _iter_tensors(traced_out)))
        if not same:
            _clear(model)
            raise _native.FqError("resident plan does not reproduce the fp32-boundary forward on the example input; "
                                  "plan removed (please report the model)")
    return planning.summary


class _Description(dict):
    """describe()'s {module name: Plan}.  After enable(relu6=True) it also says what became of the nn.ReLU6 modules:
    `fused_relu6s`, how many a producer fused, and `relu6_left`, {module name: why} for each one that stays torch's.  After
    enable(flatten=True) `flattened_concats` names the Concats that launch nothing of their own.  After enable(shuffle=True)
    `shuffle_left` is {module name: why} for every hooked nn.ChannelShuffle / Slice that stays torch's.  After
    enable(activations=True) `activations_left` is {module name: why} for every hooked elementwise activation that stays torch's,
    and `activations_revoked` names those among them that a first plan had accepted and the lossy-value verification took back.
    After enable(avgpool=True, sums=True) `avgpool_left` is {module name: why} for every hooked windowed nn.AvgPool2d that stays
    torch's.  After enable(concat=True, topdown=True) `topdown_left` is {module name: why} for every nearest upsampling in front
    of a NewAdd (or over a sum) that keeps the plan it had without the switch, and for every nn.Upsample that is foreign code.
    After enable(concat=True, bilinear=True) `bilinear_left` is {module name: why} for every hooked bilinear-mode nn.Upsample that
    stays torch's.  After enable(concat=True, requant=True) `requant_left` is {module name: why} for every Concat that the plain
    rule does not fully serve -- it has no integer plan, or emits fp32 for a reader -- and the re-quantising rule declines.  After
    enable(pixelshuffle=True) `pixelshuffle_left` is {module name: why} for every hooked nn.PixelShuffle / nn.PixelUnshuffle that
    stays torch's.  After enable(deconv=True) `deconv_left` is {module name: why} for every NewConvTranspose2d that stays an fp32
    producer."""
    activations_revoked = ()
    fused_relu6s = 0
    flattened_concats = ()       # names of the Concats that enable(flatten=True) deferred into their consumer's launch


for _switch, _keys, _attributes in _SWITCH_TABLE:           # every `*_left` report: empty while its switch is off
    for _attribute in _attributes:
        setattr(_Description, _attribute, {})


def describe(model):
    """{module name: Plan} of the current plan (for logs and tests); see _Description for the ReLU6 report."""
    d = _Description((name, m.__dict__["_resident"]) for name, m in model.named_modules() if "_resident" in m.__dict__)
    for attribute, value in model.__dict__.get("_fq_resident_report", {}).items():
        setattr(d, attribute, value)
    d.flattened_concats = tuple(name for name, m in model.named_modules()
                                if type(m).__name__ == "Concat" and name in d and d[name].defer)
    return d


class GraphedForward(object):
    """One forward of a model captured as a HIP graph (torch.cuda.CUDAGraph) and replayed per call.

    The integer-simulation forward is ~100 short kernels; below batch ~64 the Python / launch path, not
    the GPU, sets its rate.  Every kernel of this library is enqueued on the caller's stream without
    synchronising, so the whole forward captures as is.  The input is copied into a static buffer and the
    returned tensor is the graph's static output: it is overwritten by the next call (clone it to keep it).
    Batch shape is fixed at capture time."""

    def __init__(self, model, example_input, warmup=2):
        from . import new_quantity_op
        self.model = model
        self.static_in = example_input.detach().clone()
        new_quantity_op._xq_cache.clear()       # nothing memoised before the capture may be served inside it
        side = torch.cuda.Stream(device=example_input.device)
        side.wait_stream(torch.cuda.current_stream(example_input.device))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):
                model(self.static_in)
        torch.cuda.current_stream(example_input.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.static_out = model(self.static_in)
        new_quantity_op._xq_cache.clear()       # ... and nothing from the graph's private pool outside it

    def __call__(self, x):
        if x.shape != self.static_in.shape or x.dtype != self.static_in.dtype:
            raise _native.FqError("GraphedForward was captured for input %s %s" % (tuple(self.static_in.shape), self.static_in.dtype))
        self.static_in.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.static_out


class MultiStreamGraphs(object):
    """One batch as S HIP graphs of batch / S images replayed on S streams.

    At these layer sizes a kernel of the integer-simulation forward runs for 20-60 us, of which a third does not scale
    with the reduction depth (prologue, epilogue, the half-empty last round of workgroups, drain:
    profiles/r02d_conv_loop_ablation.txt); kernels of ONE stream run strictly one after the other, so that part is exposed
    54 times per forward.  Two independent halves of the batch on two streams let one half's kernels fill the CUs the other
    half's tail leaves idle: ResNet-50, 256 images, 3.21 ms as one graph -> 2.99 ms as two graphs of 128 (79 800 -> 85 700
    images/s; 512 images: 84 200 -> 90 500).  Three or four
    streams are slower again (the kernels get too small).  Same logits: every image goes through the same kernels."""

    def __init__(self, model, example_input, streams=2, warmup=2):
        n = int(example_input.shape[0])
        if streams < 2 or n % streams:
            raise _native.FqError("MultiStreamGraphs: the batch (%d) must split evenly over %d streams" % (n, streams))
        dev = example_input.device
        self.sizes = [n // streams] * streams
        self.graphs = [GraphedForward(model, p.contiguous(), warmup) for p in example_input.chunk(streams)]
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(streams)]

    def __call__(self, x):
        if int(x.shape[0]) != sum(self.sizes):
            raise _native.FqError("MultiStreamGraphs was captured for %d images" % sum(self.sizes))
        main = torch.cuda.current_stream(x.device)
        outs, off = [], 0
        for st, g, n in zip(self.streams, self.graphs, self.sizes):
            st.wait_stream(main)                              # x is ready
            with torch.cuda.stream(st):
                outs.append(g(x[off:off + n]))                # copy into the graph's static input + replay, on st
            off += n
        for st in self.streams:
            main.wait_stream(st)
        return torch.cat(outs)                                # (static outputs: overwritten by the next call)


def capture(model, example_input, warmup=2, streams=1):
    """HIP-graph capture of `model`'s forward at the shape of `example_input` (see GraphedForward); streams > 1: the batch
    split into that many graphs replayed concurrently (see MultiStreamGraphs)."""
    if streams > 1:
        return MultiStreamGraphs(model, example_input, streams, warmup)
    return GraphedForward(model, example_input, warmup)
