"""Layers of the MoCo-v2 R50 hot path, executed by libpassl_hip.so.

PyTorch provides parameter storage and the autograd tape only: every ``autograd.Function``
below launches hand-written HIP kernels through the C ABI (passl_amd/hip/ops.py) in both
directions.  Activations are NHWC in the compute dtype (bf16, or fp32 for parity runs).

Storage model (EncoderArena): all parameters and BN statistics of one encoder live in ONE flat
fp32 buffer, each conv weight physically [K][R][S][C] and each Linear weight [out][in]
(K-contiguous rows = the B operand of the implicit GEMM); the ``nn.Parameter`` objects are
strided *views* with the reference's logical shapes ([Cout,Cin,kh,kw], Linear [in,out]) so
``state_dict()`` matches the reference layout.  Gradients are written by the
kernels straight into a flat fp32 gradient buffer (``p.grad`` are views of it), so the key-
encoder EMA, the optimizer and the DP all-reduce are single launches over flat memory.

Reference semantics mirrored here: paddle.nn.Conv2D(bias_attr=False), BatchNorm2D (momentum 0.9,
eps 1e-5, biased running var, ``_use_global_stats``), MaxPool2D(3,2,1), AdaptiveAvgPool2D(1),
Linear — as used by passl_v110/modeling/backbones/resnetimagenet.py:111-253 and
passl_v110/modeling/necks/base_neck.py:68-97.
"""
import os
from types import SimpleNamespace

import torch
import torch.nn as tnn
from torch.autograd import Function

from . import config, ops, streams
from . import plan as P
from .packer import WeightPacker


class Layer(tnn.Module):
    """torch Module with the few paddle.nn.Layer spellings the reference's code relies on."""

    def sublayers(self, include_self=False):
        mods = list(self.modules())
        return mods if include_self else mods[1:]

    def set_state_dict(self, sd, *a, **k):
        return self.load_state_dict(sd, *a, **k)


def _need_rt(layer):
    if getattr(layer, '_rt', None) is None:
        raise RuntimeError('%s is not attached to an EncoderArena (call EncoderArena(encoder) after '
                           'building the model)' % type(layer).__name__)
    return layer._rt


class GradSlot:
    """Hand-off of ONE gradient tensor between two backward nodes of a residual fork.

    A block input x feeds conv1 and the identity (or downsample) branch, so autograd would add the
    two input gradients with an extra elementwise kernel.  Instead the branch whose backward runs
    first (bn3's identity gradient, or the downsample conv's dx) `put`s its tensor here and
    returns None to autograd; conv1's backward `take`s it and the data-gradient kernel adds it in
    its epilogue.  The order is fixed by the graph (conv1's backward depends on bn3's), and it is
    checked: a `take` from a slot that was armed but never filled raises instead of silently
    dropping a gradient."""

    __slots__ = ('armed', 'grad', 'ready')

    def __init__(self):
        self.armed = False
        self.grad = None
        self.ready = None

    def arm(self):
        self.armed = True

    def put(self, g):
        if not self.armed or self.grad is not None:
            raise RuntimeError('GradSlot.put: slot not armed or already filled')
        self.grad = g
        # the two ends may run on different streams (a downsample branch on the side stream,
        # hip/streams.py): the taker waits for the producer's launches
        self.ready = streams.record_event(torch.cuda.current_stream(g.device)) if g.is_cuda else None

    def take(self):
        if not self.armed:
            return None
        if self.grad is None:
            raise RuntimeError('GradSlot.take: the residual-branch gradient has not been produced '
                               'yet (autograd executed the fork in an unexpected order)')
        g, self.grad, self.armed = self.grad, None, False
        if self.ready is not None:
            # g may come from the side stream's pool (a forked downsample branch): ordered by the event; its
            # block is recycled behind later side-stream work only, all of which waits on main-stream events
            # recorded after this launch (hip/streams.py, "Memory") — no record_stream
            streams.wait_event(torch.cuda.current_stream(g.device), self.ready)
            self.ready = None
        return g


class BNLink:
    """Hand-off between a training-mode BatchNorm(+ReLU) layer and the ONE convolution that consumes
    its output.  The BatchNorm's forward records what its backward statistics need (its input y, the
    batch statistics, the ReLU mask source); the consumer's data-gradient launch — which produces
    exactly the gradient w.r.t. the BatchNorm output — masks that gradient and writes the per-tile
    (sum g, sum g*xhat) slab in its epilogue (csrc/igemm_epi.h), and reports it here.  The BatchNorm's
    backward then skips its reduce pass, and the gradient it receives is already g."""

    __slots__ = ('y', 'st', 'mask', 'relu_mode', 'fused', 'res_link')

    def __init__(self, y, st, mask, relu_mode, res_link=None):
        self.y, self.st, self.mask, self.relu_mode = y, st, mask, relu_mode
        self.fused = None            # (slab, tiles) once a data-gradient launch has done the work
        # the BNLink of the BatchNorm (without ReLU) whose output is this layer's RESIDUAL input and has no other
        # consumer — a bottleneck block's downsample branch: relu(bn3(y3) + bn_ds(y_ds)).  The masked gradient g of
        # this layer's output is then the output gradient of that BatchNorm as well, and the data-gradient launch that
        # reduces (sum g, sum g*xhat) for this layer can do it for that one in the same pass (conv desc bnb2_*).
        self.res_link = res_link


def bn_link(t):
    """The BNLink riding on a BatchNorm output tensor (None for anything else)."""
    return getattr(t, '_passl_bn_link', None)


class BNPending:
    """The forward twin of BNLink: a training-mode BatchNorm + ReLU whose ONE consumer is a 1x1 convolution of the
    register-staged kernel does not run its apply pass.  Its forward finalizes the statistics, allocates the output z and
    lets this object ride on it: (y, scale, shift).  The consumer's forward launch reads y, applies the BatchNorm to the
    operand on its way into the kernel and writes z (ops.conv_igemm(apro=...)) — one pass over the tensor less, one
    launch less.  Until then z holds nothing: the tensor must reach that convolution and nothing else.  Where the library
    does not serve the launch in that form, the consumer runs the apply pass itself, then the plain convolution."""

    __slots__ = ('y', 'scale', 'shift')

    def __init__(self, y, scale, shift):
        self.y, self.scale, self.shift = y, scale, shift


def bn_pending(t):
    """The BNPending riding on a BatchNorm output tensor whose apply pass is still to be done (None otherwise)."""
    return getattr(t, '_passl_bn_pending', None)


class DyLink:
    """BNPending's backward twin, between a convolution and the BatchNorm that reads its output.  When that BatchNorm's
    output gradient arrives masked and reduced (BNLink.fused), its backward runs the finalize only, allocates dy and
    `put`s (g, y, coef, dy) here; the convolution's data-gradient launch — the one reader of dy besides the weight
    gradient — computes dy from g and y on its way in and writes it (ops.conv_igemm(apro=...)); the weight gradient,
    launched after it, reads dy as before.  The link rides on the convolution's output tensor (dy_link) for the shapes
    whose data gradient is one dense launch with a single 64-column block, and is used only by a BatchNorm that is told
    it is that tensor's sole reader (_BatchNormBase.forward(sole_reader=True))."""

    __slots__ = ('pending',)

    def __init__(self):
        self.pending = None

    def put(self, g, y, coef, dy):
        self.pending = (g, y, coef, dy)

    def take(self, dy):
        p, self.pending = self.pending, None
        if p is not None and p[3].data_ptr() != dy.data_ptr():
            raise RuntimeError('DyLink: the gradient that reached the convolution is not the one its BatchNorm deferred')
        return p


def dy_link(t):
    """The DyLink riding on a convolution output tensor (None for anything else)."""
    return getattr(t, '_passl_dy_link', None)


def _apply_in_consumer(conv, y, residual, relu, stats):
    """Shapes for which a BatchNorm leaves its apply pass to `conv` (include/passl_hip.h: passl_hip_conv_igemm_apro,
    PASSL_APRO_BN_FWD) where config.igemm_a_bn allows it; the library has the last word (kernel selection)."""
    g = conv.geom
    return (relu and residual is None and stats is not None and y.dtype == torch.bfloat16 and not conv.is_stem and
            g.k == 1 and g.stride == 1 and g.pad == 0 and g.cin == y.shape[-1] and g.cin % 64 == 0 and g.cin < 512 and
            g.cout > 64 and config.igemm_a_bn(g.cin))


class WgradLink:
    """Hand-off in the other direction, for the stem: the layer that PRODUCES a convolution's output gradient (the fused
    BatchNorm + ReLU + max-pool backward, two launches from the end of a backward pass) launches that convolution's
    weight gradient itself, piece of the batch by piece, each on the side stream as soon as the apply pass has written
    the piece (`launch`), and says so (`done`); the convolution's own backward then has nothing left to launch."""

    __slots__ = ('launch', 'done')

    def __init__(self):
        self.launch = None           # launch(dy, n0, n1, i, parts): images n0..n1 of dy (piece i) are written; set by the convolution
        self.done = False            # set by the producer of dy once every piece has been handed over


def wgrad_link(t):
    """The WgradLink riding on a convolution output tensor (None for anything else)."""
    return getattr(t, '_passl_wgrad_link', None)


# =============================================================================== conv
def _stem_wgrad(layer, pl, x, dy, tmp):
    """The stem filter is padded to [K][7][8 taps][4 channels] for the kernel; `tmp` (zeroed) collects its gradient."""
    ops.conv_wgrad(pl.wd, x, dy.reshape(-1, layer.geom.cout), tmp)


def _stem_wgrad_finish(layer, tmp):
    """... which goes back into the dense [K][7][7][3] slot of the flat gradient buffer."""
    ops.unpad_add(tmp, layer._rt.dw, layer.geom.cout, 7, 7, 3, P.STEM_ROW // 4, 4)


class _ConvFn(Function):
    @staticmethod
    def forward(ctx, x, weight, layer, hw, stats, add_slot, sink_slot, producer, wlink=None, pending=None,
                dylink=None):
        rt = _need_rt(layer)
        N = x.shape[0]
        pl = layer._plan(N, hw[0], hw[1])
        y = torch.empty(N, pl.fd.OP, pl.fd.OQ, layer.geom.cout, dtype=x.dtype, device=x.device)
        slab = stats[0] if stats is not None else None
        done = None
        if pending is not None:
            # x is the still-empty output of a BatchNorm (BNPending): this launch applies it and fills x
            done = ops.conv_igemm(pl.fd, pending.y, rt.w_fwd, y, stats=slab,
                                  apro=dict(mode=1, scale=pending.scale, shift=pending.shift, out=x))
            if done is None:
                ops.bn_apply(pending.y, pending.scale, pending.shift, None, True, out=x)
        if done is None:
            ops.conv_igemm(pl.fd, x, rt.w_fwd, y, stats=slab)
        if any(ctx.needs_input_grad):
            rt.arena.expect_grad(rt.indices)
        ctx.save_for_backward(x)
        ctx.layer, ctx.pl, ctx.hw = layer, pl, hw
        ctx.add_slot, ctx.sink_slot, ctx.producer = add_slot, sink_slot, producer
        # latched: forward and backward of one step agree about the side stream even if the allocator-pressure
        # back-off of streams.enabled() flips in between
        ctx.side = streams.enabled(x)
        ctx.wlink = None
        ctx.dylink = dylink
        if wlink is not None and ctx.side and any(ctx.needs_input_grad):
            # the producer of dy may launch the weight gradient in pieces of the batch (WgradLink)
            ctx.wlink = wlink
            state = {}

            def piece(dy_all, n0, n1, tmp):
                _stem_wgrad(layer, layer._plan(n1 - n0, hw[0], hw[1]), x[n0:n1], dy_all[n0:n1], tmp)

            def launch(dy_all, n0, n1, i, parts):
                dev = dy_all.device
                on_main = parts > 1 and config.stem_wgrad_main_last()      # the last piece
                if on_main and i == parts - 1:
                    # the last piece on THIS stream, into a buffer of its own; dW += it once the side stream's pieces
                    # are in (same order every step)
                    tmp = ops.zeros(layer.geom.cout, P.STEM_K * P.STEM_ROW, dtype=torch.float32, device=dev)
                    piece(dy_all, n0, n1, tmp)
                    streams.wait_stream(torch.cuda.current_stream(dev), streams.side_stream(dev))
                    _stem_wgrad_finish(layer, tmp)
                    return
                with streams.on_side(dev, reads=(x, dy_all), in_backward=True):
                    if 'tmp' not in state:
                        state['tmp'] = ops.zeros(layer.geom.cout, P.STEM_K * P.STEM_ROW, dtype=torch.float32, device=dev)
                    piece(dy_all, n0, n1, state['tmp'])
                    if i == parts - (2 if on_main else 1):
                        _stem_wgrad_finish(layer, state.pop('tmp'))
            wlink.launch = launch
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer, pl = ctx.layer, ctx.pl
        rt = layer._rt
        g = layer.geom
        streams.autograd_node_entry(dy.device)
        dy = dy.contiguous()
        dx = None
        # dy may still be empty (DyLink): the data-gradient launch below fills it, or the apply pass does, here
        late = ctx.dylink.take(dy) if ctx.dylink is not None else None
        if late is not None and not (ctx.needs_input_grad[0] and len(pl.dds) == 1 and not pl.dgrad_zero):
            ops.bn_bwd_apply_fused(late[0], late[1], late[2], dy)
            late = None
        if ctx.needs_input_grad[0]:
            N = x.shape[0]
            alloc = ops.zeros if pl.dgrad_zero else torch.empty
            dx = alloc(N, ctx.hw[0], ctx.hw[1], g.cin, dtype=dy.dtype, device=dy.device)
            extra = ctx.add_slot.take() if ctx.add_slot is not None else None
            if extra is not None and (len(pl.dds) != 1 or pl.dgrad_zero):
                raise RuntimeError('residual-gradient fusion needs a single dense data-gradient conv')
            link = ctx.producer
            fuse = (link is not None and dy.dtype == torch.bfloat16 and not pl.dgrad_zero and
                    ctx.sink_slot is None and config.fused_bn_backward())
            slab, slab2, off = None, None, 0
            if fuse:
                tiles = sum(ops.conv_tiles(d) for d in pl.dds)
                slab = torch.empty(ops.bn_partial_floats(tiles, g.cin, False), dtype=torch.float32,
                                   device=dy.device)
                # the downsample branch's BatchNorm behind the same gradient: reduced by this launch too (the
                # instantiation covers dense 1x1 launches of at least 128 columns: conv1 of the block that follows)
                rl = link.res_link
                if (rl is not None and rl.relu_mode == 0 and rl.y is not None and config.fused_bn_backward2() and
                        len(pl.dds) == 1 and g.k == 1 and g.stride == 1 and g.pad == 0 and g.cout % 64 == 0 and
                        g.cin >= 128):
                    slab2 = torch.empty(ops.bn_partial_floats(tiles, g.cin, False), dtype=torch.float32,
                                        device=dy.device)
            for d in pl.dds:
                bnb = None
                if fuse:
                    bnb = dict(y=link.y, mask=link.mask, mean=link.st[0], invstd=link.st[1],
                               scale=link.st[2], shift=link.st[3], relu=link.relu_mode, partial=slab,
                               tile_off=off)
                    if slab2 is not None:
                        bnb.update(y2=link.res_link.y, mean2=link.res_link.st[0], invstd2=link.res_link.st[1],
                                   partial2=slab2)
                    off += ops.conv_tiles(d)
                if late is not None:
                    done = ops.conv_igemm(d, late[0], rt.w_dgrad[id(d.pack)], dx, residual=extra, bnb=bnb,
                                          apro=dict(mode=2, a2=late[1], coef=late[2], out=dy))
                    if done is None:
                        ops.bn_bwd_apply_fused(late[0], late[1], late[2], dy)
                    late = None
                    if done is not None:
                        continue
                ops.conv_igemm(d, dy, rt.w_dgrad[id(d.pack)], dx, residual=extra, bnb=bnb)
                if slab2 is not None and not bnb.get('partial2_done', False):
                    slab2 = None          # the library took the launch without the second layer (ops.conv_igemm)
            if fuse:
                link.fused = (slab, off)
                if slab2 is not None:
                    link.res_link.fused = (slab2, off)
            if ctx.sink_slot is not None:
                ctx.sink_slot.put(dx)
                dx = None
        def wgrad():
            if layer.is_stem:
                tmp = ops.zeros(g.cout, P.STEM_K * P.STEM_ROW, dtype=torch.float32, device=dy.device)
                _stem_wgrad(layer, pl, x, dy, tmp)
                _stem_wgrad_finish(layer, tmp)
            else:
                ops.conv_wgrad(pl.wd, x, dy.view(-1, g.cout), rt.dw)
        wl = ctx.wlink
        if wl is not None:
            wl.launch = None                      # (the closure holds x)
        if wl is not None and wl.done:
            pass                                  # launched by the producer of dy, piece by piece
        elif ctx.side:
            # dW feeds only the optimizer: off the dgrad -> BatchNorm-backward chain (hip/streams.py)
            rows = config.side_urgent_rows()
            streams.side_later(dy.device, wgrad, reads=(x, dy), urgent=rows > 0 and dy.numel() // g.cout >= rows)
        else:
            wgrad()
        rt.arena.grad_ready(rt.indices)
        return dx, None, None, None, None, None, None, None, None, None, None


class Conv2D(Layer):
    """Bias-free 2-D convolution, NHWC activations, weight logically [Cout,Cin,kh,kw]."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1,
                 groups=1, bias_attr=False, **_):
        super().__init__()
        assert bias_attr is False, 'only bias-free convs are on the hot path'
        assert dilation == 1 and groups == 1
        self.geom = P.ConvGeom(in_channels, out_channels, kernel_size, stride, padding)
        self.is_stem = (in_channels, kernel_size, stride, padding) == (3, 7, 2, 3)
        self.weight = tnn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size,
                                                device=config.get_device()))
        self._rt = None
        self._plans = {}

    def _plan(self, N, H, W):
        key = (N, H, W)
        pl = self._plans.get(key)
        if pl is None:
            rt = _need_rt(self)
            g = self.geom
            if self.is_stem:
                fd = P.stem_desc(g.cout, N, H, W)
                pl = SimpleNamespace(fd=fd, wd=fd, dds=[], dgrad_zero=False)
            else:
                dds, skipped = ([], False)
                if rt.dgrad_packs is not None:
                    dds, skipped = P.dgrad_plan(g, N, H, W, packs=rt.dgrad_packs)
                pl = SimpleNamespace(fd=P.fwd_desc(g, N, H, W), wd=P.wgrad_desc(g, N, H, W),
                                     dds=dds, dgrad_zero=skipped)
            self._plans[key] = pl
        return pl

    def forward(self, x, hw=None, want_stats=False, add_slot=None, sink_slot=None, producer=None, pending=None):
        """x: NHWC compute-dtype tensor (the stem takes the zero-padded image + hw=(H, W)).
        want_stats: also return the fused BatchNorm statistics slab written by the conv epilogue
        ((slab, tiles); None when the dtype has no fused path) -> (y, stats).
        add_slot / sink_slot: residual-fork gradient hand-off (GradSlot): this conv's backward adds
        the slot's tensor to dx in the kernel epilogue / deposits its dx there instead of
        returning it.
        producer: BNLink of the BatchNorm layer whose output is x, given ONLY when this conv's
        data-gradient launch produces the complete gradient of x (sole consumer, or the residual fork
        folded in through add_slot): the launch then also does that BatchNorm's backward reduction.
        pending: BNPending of x when the BatchNorm that produced it left its apply pass to this conv (bn_pending(x))."""
        if hw is None:
            hw = (x.shape[1], x.shape[2])
        stats = None
        if want_stats and x.dtype == torch.bfloat16 and config.fused_bn_stats():
            stats = ops.conv_stats_buffer(self._plan(x.shape[0], hw[0], hw[1]).fd, x.device)
        wlink = WgradLink() if (self.is_stem and config.stem_wgrad_parts() > 1) else None
        g = self.geom
        dylink = DyLink() if (torch.is_grad_enabled() and x.dtype == torch.bfloat16 and not self.is_stem and
                              g.k == 1 and g.stride == 1 and g.pad == 0 and g.cin <= 64 and g.cout % 64 == 0 and
                              g.cout < 512 and config.fused_bn_backward() and config.igemm_a_bnb(g.cout)) else None
        y = _ConvFn.apply(x, self.weight, self, hw, stats, add_slot, sink_slot, producer, wlink, pending, dylink)
        if dylink is not None:
            y._passl_dy_link = dylink
        if wlink is not None and wlink.launch is not None:
            y._passl_wgrad_link = wlink
        return (y, stats) if want_stats else y

    @torch.no_grad()
    def infer(self, x, bn=None, residual=None, relu=False, hw=None):
        """conv + (BatchNorm with running stats) + residual + ReLU in ONE kernel (epilogue)."""
        rt = _need_rt(self)
        if hw is None:
            hw = (x.shape[1], x.shape[2])
        N = x.shape[0]
        pl = self._plan(N, hw[0], hw[1])
        y = torch.empty(N, pl.fd.OP, pl.fd.OQ, self.geom.cout, dtype=x.dtype, device=x.device)
        scale = shift = None
        if bn is not None:
            scale, shift = bn.infer_affine()
        ops.conv_igemm(pl.fd, x, rt.w_fwd, y, scale=scale, shift=shift, residual=residual, relu=relu)
        return y


# =============================================================================== batch norm
def _collectives_active():
    from ..core.sync_utils import collectives_active
    return collectives_active()


def convert_sync_batchnorm(module):
    """paddle.nn.SyncBatchNorm.convert_sync_batchnorm: every BatchNorm of `module` computes its training statistics
    over the batches of ALL data-parallel ranks from now on (no-op without a process group)."""
    for m in module.modules():
        if isinstance(m, _BatchNormBase):
            m._sync = True
    return module


class _BNActFn(Function):
    @staticmethod
    def forward(ctx, y, gamma, beta, residual, layer, relu, partial, res_slot, link_box, res_link=None, pend_box=None,
                dylink=None):
        has_res = residual is not None
        # SyncBatchNorm (convert_sync_batchnorm): statistics over every rank's batch when a process group is up
        ctx.sync = bool(getattr(layer, '_sync', False)) and _collectives_active()
        z, st, mask = ops.bn_train_fwd(y, gamma.detach(), beta.detach(), layer._mean,
                                       layer._variance, residual, relu, layer._momentum,
                                       layer._epsilon, partial=partial,
                                       want_mask=relu and has_res, sync=ctx.sync, apply=pend_box is None)
        if pend_box is not None:
            # statistics only: the consumer convolution applies them and fills z (BNPending)
            z = torch.empty_like(y)
            pend_box[0] = BNPending(y, st[2], st[3])
        # ReLU mask for the backward: recomputed from y (no residual) or the bit mask (residual):
        # the output z is never re-read by this layer's backward.
        ctx.relu_mode = 0 if not relu else (3 if has_res else 2)
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        ctx.save_for_backward(y, st, mask)
        ctx.layer, ctx.has_res, ctx.res_slot = layer, has_res, res_slot
        ctx.link = None
        ctx.dylink = dylink
        if link_box is not None:
            ctx.link = link_box[0] = BNLink(y, st, mask, ctx.relu_mode,
                                            res_link if (has_res and ctx.relu_mode == 3 and res_slot is None) else None)
        return z

    @staticmethod
    def backward(ctx, dz):
        y, st, mask = ctx.saved_tensors
        layer = ctx.layer
        streams.autograd_node_entry(dz.device)
        if layer.affine:
            for p in (layer.weight, layer.bias):
                if p.grad is None:
                    p.grad = ops.zeros_like(p)
            gamma, dgamma, dbeta = layer.weight.detach(), layer.weight.grad, layer.bias.grad
        else:
            gamma, dgamma, dbeta = layer._const[0], layer._dscratch[0], layer._dscratch[1]
        want_dres = ctx.has_res and (ctx.needs_input_grad[3] or ctx.res_slot is not None)
        # the consumer conv's data-gradient launch may already have masked dz and reduced it
        fused = ctx.link.fused if ctx.link is not None else None
        if ctx.link is not None:
            ctx.link.y = ctx.link.st = ctx.link.mask = ctx.link.fused = ctx.link.res_link = None   # drop the references
        if fused is not None and fused[0].is_cuda:
            # the slab may have been written by a launch on ANOTHER stream (a downsample branch's layer runs its
            # backward on the side stream; its slab comes from the main stream's data-gradient launch and pool)
            fused[0].record_stream(torch.cuda.current_stream(dz.device))
        dz = dz.contiguous()
        # gradient already masked and reduced, and the convolution that produced y takes dx as a pending operand (DyLink)
        defer = (fused is not None and ctx.dylink is not None and ctx.needs_input_grad[0] and
                 dz.dtype == torch.bfloat16)
        out = ops.bn_bwd(dz, mask, y, gamma, st[0], st[1], dgamma, dbeta, relu=ctx.relu_mode,
                         want_dres=want_dres, scale=st[2], shift=st[3], fused=fused, sync=ctx.sync, defer=defer)
        dx, dres = out[0], out[1]
        if defer:
            ctx.dylink.put(dz, y, out[2], dx)
        if ctx.res_slot is not None:
            ctx.res_slot.put(dres)
            dres = None
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, dres, None, None, None, None, None, None, None, None


class _BatchNormBase(Layer):
    """BatchNorm over the channel (last) axis of NHWC rows.  ``_mean`` / ``_variance`` keep the
    reference's state_dict key names; ``_use_global_stats`` is what freeze_batchnorm_statictis
    (passl_v110/modules/freeze.py:18-23) flips on the key encoder."""

    def __init__(self, num_features, momentum=0.9, epsilon=1e-05, weight_attr=None,
                 bias_attr=None, data_format='NCHW', use_global_stats=None, name=None):
        super().__init__()
        dev = config.get_device()
        self._momentum, self._epsilon = momentum, epsilon
        self._use_global_stats = use_global_stats
        self.num_features = num_features
        # weight_attr=False / bias_attr=False (both or neither): no gamma / beta (the last BatchNorm of MoCo-v3's
        # projector and predictor, passl/models/mocov3.py:152-157).  The kernels read constant 1 / 0 vectors and
        # write the unused d-gamma / d-beta into a scratch pair; neither shows up in parameters() or state_dict().
        if (weight_attr is False) != (bias_attr is False):
            raise NotImplementedError('BatchNorm with only one of weight / bias')
        self.affine = weight_attr is not False
        if self.affine:
            self.weight = tnn.Parameter(torch.ones(num_features, device=dev))
            self.bias = tnn.Parameter(torch.zeros(num_features, device=dev))
        else:
            self.weight = self.bias = None
            self.register_buffer('_const', torch.stack([torch.ones(num_features, device=dev),
                                                        torch.zeros(num_features, device=dev)]), persistent=False)
            self.register_buffer('_dscratch', torch.zeros(2, num_features, device=dev), persistent=False)
        self.register_buffer('_mean', torch.zeros(num_features, device=dev))
        self.register_buffer('_variance', torch.ones(num_features, device=dev))
        self._rt = None

    def uses_global_stats(self):
        return bool(self._use_global_stats) if self._use_global_stats is not None \
            else (not self.training)

    def infer_affine(self):
        """(scale, shift) of y = x*scale + shift with the running statistics."""
        rt = self._rt
        if rt is not None and rt.arena.bn_affine is not None:
            s, e = rt.bn_slice
            return rt.arena.bn_affine[0][s:e], rt.arena.bn_affine[1][s:e]
        gamma, beta = self.gamma_beta()
        scale = gamma * torch.rsqrt(self._variance + self._epsilon)
        return scale, beta - self._mean * scale

    def gamma_beta(self):
        if self.affine:
            return self.weight.detach(), self.bias.detach()
        return self._const[0], self._const[1]

    def forward(self, y, residual=None, relu=False, stats=None, res_slot=None, res_link=None, consumer=None,
                sole_reader=False):
        """stats: fused statistics from the producing conv's epilogue (Conv2D.forward(...,
        want_stats=True)); res_slot: GradSlot that receives the residual branch's gradient; res_link: bn_link of the
        residual when it is the output of a BatchNorm that nothing else consumes (BNLink.res_link); consumer: the Conv2D
        that is the ONLY reader of the output and is called with pending=bn_pending(output) (BNPending);
        sole_reader: y is the output of a Conv2D and this layer is its ONLY reader, so this layer's backward may leave
        its apply pass to that convolution's data-gradient launch (DyLink, riding on y).  Never set it for a tensor
        that something else reads as well: autograd would add the still empty gradient to the other reader's."""
        if self.uses_global_stats():
            if torch.is_grad_enabled() and (y.requires_grad or (self.affine and self.weight.requires_grad)):
                raise NotImplementedError('frozen BatchNorm inside a differentiated graph is not on '
                                          'the MoCo hot path (key encoder runs under no_grad)')
            scale, shift = self.infer_affine()
            return ops.bn_apply(y, scale, shift, residual, relu)
        # the output carries a BNLink so that a sole-consumer conv can take over the backward reduction
        box = [None] if (torch.is_grad_enabled() and y.dtype == torch.bfloat16 and
                         config.fused_bn_backward()) else None
        gamma, beta = (self.weight, self.bias) if self.affine else (self._const[0], self._const[1])
        pend = [None] if (consumer is not None and _apply_in_consumer(consumer, y, residual, relu, stats)) else None
        z = _BNActFn.apply(y, gamma, beta, residual, self, relu, stats, res_slot, box, res_link, pend,
                           dy_link(y) if sole_reader else None)
        if box is not None and box[0] is not None:
            z._passl_bn_link = box[0]
        if pend is not None:
            z._passl_bn_pending = pend[0]
        return z


class BatchNorm2D(_BatchNormBase):
    pass


class BatchNorm1D(_BatchNormBase):
    pass


# =============================================================================== pooling
class _MaxPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        y, idx = ops.maxpool_fwd(x)
        ctx.save_for_backward(idx)
        ctx.hw = (x.shape[1], x.shape[2])
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        return ops.maxpool_bwd(dy.contiguous(), idx, ctx.hw[0], ctx.hw[1])


class _BNReluMaxPoolFn(Function):
    """Training-mode BatchNorm + ReLU + MaxPool2D(3, 2, 1) in one pass per direction (csrc/stem_pool.hip): the stem of
    the trainable trunk (resnetimagenet.py:196-198).  Saves the BatchNorm input, the batch statistics and one index
    byte per pooled element; neither the BatchNorm output nor the pool's input gradient is ever written."""

    @staticmethod
    def forward(ctx, y, gamma, beta, layer, partial, wlink=None):
        _, st, _ = ops.bn_train_fwd(y, gamma.detach(), beta.detach(), layer._mean, layer._variance, None, True,
                                    layer._momentum, layer._epsilon, partial=partial, apply=False)
        out, idx = ops.bn_relu_maxpool_fwd(y, st)
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        ctx.save_for_backward(y, st, idx)
        ctx.layer, ctx.wlink = layer, wlink
        return out

    @staticmethod
    def backward(ctx, dout):
        y, st, idx = ctx.saved_tensors
        layer, wl = ctx.layer, ctx.wlink
        streams.autograd_node_entry(dout.device)
        # These launches and the stem's weight gradient are the tail of the backward pass: weight gradients still queued
        # for the side stream go there now, next to them, not behind them.
        if config.stem_tail_flush():
            streams.flush_side(dout.device)
        for p in (layer.weight, layer.bias):
            if p.grad is None:
                p.grad = ops.zeros_like(p)
        piecewise = wl is not None and wl.launch is not None and not wl.done
        dx = ops.bn_relu_maxpool_bwd(dout.contiguous(), idx, y, layer.weight.detach(), st, layer.weight.grad,
                                     layer.bias.grad, parts=config.stem_wgrad_parts() if piecewise else 1,
                                     on_part=wl.launch if piecewise else None)
        if piecewise:
            wl.done = True
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, None, None, None


def bn_relu_maxpool(bn, y, stats=None):
    """bn(y, relu=True) followed by MaxPool2D(3, 2, 1).  One fused pass per direction when `bn` computes batch
    statistics of this rank (training mode, affine, no SyncBatchNorm) and the shape is covered; the two layers
    otherwise."""
    fused = (config.fused_stem_pool() and torch.is_grad_enabled() and not bn.uses_global_stats() and bn.affine and
             not (getattr(bn, '_sync', False) and _collectives_active()) and y.is_cuda and
             ops.bn_relu_maxpool_supported(y))
    if not fused:
        return _MaxPoolFn.apply(bn(y, relu=True, stats=stats))
    return _BNReluMaxPoolFn.apply(y, bn.weight, bn.bias, bn, stats, wgrad_link(y))


class MaxPool2D(Layer):
    def __init__(self, kernel_size=3, stride=2, padding=1):
        super().__init__()
        assert (kernel_size, stride, padding) == (3, 2, 1), 'only the ResNet stem pool is built'

    def forward(self, x):
        return _MaxPoolFn.apply(x)


class _AvgPoolFn(Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[1], x.shape[2])
        return ops.avgpool_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return ops.avgpool_bwd(dy.contiguous(), ctx.hw[0], ctx.hw[1])


class AdaptiveAvgPool2D(Layer):
    def __init__(self, output_size=(1, 1)):
        super().__init__()
        assert tuple(output_size) == (1, 1) if not isinstance(output_size, int) else output_size == 1

    def forward(self, x):
        """[N,H,W,C] -> [N,C]"""
        return _AvgPoolFn.apply(x)


class ReLU(Layer):
    """Marker layer: ReLU is always fused into the producing kernel's epilogue
    (BatchNorm-apply, conv epilogue or Linear epilogue)."""

    def forward(self, x):
        raise RuntimeError('ReLU is fused into the preceding layer on the HIP path')


# =============================================================================== linear
class _LinearFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, layer, relu, out_f32, residual):
        rt = _need_rt(layer)
        N = x.shape[0]
        pl = layer._plan(N)
        y = torch.empty(N, layer.out_features, dtype=torch.float32 if out_f32 else x.dtype,
                        device=x.device)
        ops.conv_igemm(pl.fd, x, rt.w_fwd, y, shift=bias.detach() if bias is not None else None,
                       relu=relu, out_f32=out_f32, residual=residual)
        if any(ctx.needs_input_grad):
            rt.arena.expect_grad(rt.indices)
        ctx.save_for_backward(x, y if relu else None)
        ctx.layer, ctx.pl, ctx.relu = layer, pl, relu
        ctx.has_res = residual is not None
        ctx.side = streams.enabled(x)              # latched for the backward (see _ConvFn)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        layer, pl = ctx.layer, ctx.pl
        rt = layer._rt
        dy = dy.contiguous()
        if dy.dtype != x.dtype:
            dy = ops.cast_to(dy, x.dtype)
        if ctx.relu:
            dy = ops.relu_bwd(dy, y)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape[0], layer.in_features, dtype=x.dtype, device=x.device)
            d = pl.dds[0]
            ops.conv_igemm(d, dy, rt.w_dgrad[id(d.pack)], dx)
        want_bias = layer.bias is not None and layer.bias.requires_grad
        if ctx.side and not config.side_reductions():
            streams.side_later(dy.device, lambda: ops.conv_wgrad(pl.wd, x, dy, rt.dw), reads=(x, dy))
            if want_bias:
                ops.colsum_into(dy, layer.bias.grad, accumulate=True)
        elif ctx.side:
            # the bias gradient (column sums of dy) rides along: like dW it feeds only the optimizer, and its two small
            # launches are latency-bound — off the data-gradient chain (MAE: 83 of them per step, 1.1 ms)
            bias_grad = layer.bias.grad if want_bias else None

            def side_work():
                ops.conv_wgrad(pl.wd, x, dy, rt.dw)
                if want_bias:
                    ops.colsum_into(dy, bias_grad, accumulate=True)     # straight into the arena's gradient
            streams.side_later(dy.device, side_work, reads=(x, dy))
        else:
            ops.conv_wgrad(pl.wd, x, dy, rt.dw)
            if want_bias:
                ops.colsum_into(dy, layer.bias.grad, accumulate=True)
        rt.arena.grad_ready(rt.indices)
        # y = x W + b + residual: the residual branch's gradient is dy itself
        return dx, None, None, None, None, None, (dy if ctx.has_res else None)


class Linear(Layer):
    """y = x W + b with W logically [in, out] (the reference's paddle.nn.Linear layout)."""

    def __init__(self, in_features, out_features, weight_attr=None, bias_attr=None, name=None):
        super().__init__()
        dev = config.get_device()
        self.in_features, self.out_features = in_features, out_features
        self.geom = P.ConvGeom(in_features, out_features, 1, 1, 0)
        self.weight = tnn.Parameter(torch.empty(in_features, out_features, device=dev))
        self.bias = None if bias_attr is False else tnn.Parameter(torch.zeros(out_features, device=dev))
        self._rt = None
        self._plans = {}

    def _plan(self, N):
        pl = self._plans.get(N)
        if pl is None:
            rt = _need_rt(self)
            dds = []
            if rt.dgrad_packs is not None:
                dds, _ = P.dgrad_plan(self.geom, N, 1, 1, packs=rt.dgrad_packs)
            pl = SimpleNamespace(fd=P.fwd_desc(self.geom, N, 1, 1), wd=P.wgrad_desc(self.geom, N, 1, 1),
                                 dds=dds)
            self._plans[N] = pl
        return pl

    def forward(self, x, relu=False, out_f32=False, residual=None):
        """residual: tensor shaped like the output, added in the GEMM epilogue (before the ReLU)."""
        return _LinearFn.apply(x, self.weight, self.bias, self, relu, out_f32, residual)


class _ToComputeFn(Function):
    """fp32 rows -> compute dtype (bf16) with a HIP cast kernel; gradient comes back as fp32."""

    @staticmethod
    def forward(ctx, x):
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        ops.cast_bf16(x.contiguous().view(-1), y.view(-1))
        return y

    @staticmethod
    def backward(ctx, dy):
        return ops.cast_f32(dy)


class _ToF32Fn(Function):
    """Compute-dtype rows -> fp32 with a HIP cast kernel; the gradient goes back in the rows' dtype."""

    @staticmethod
    def forward(ctx, x):
        ctx.dtype = x.dtype
        return ops.cast_f32(x.contiguous())

    @staticmethod
    def backward(ctx, dy):
        return ops.cast_to(dy.contiguous(), ctx.dtype)


def to_f32(x):
    """Widen a compute-dtype activation to fp32 (identity for fp32)."""
    return x if x.dtype == torch.float32 else _ToF32Fn.apply(x)


def to_compute(x, dtype):
    """Cast an fp32 activation to the compute dtype (identity for fp32 compute)."""
    if dtype == torch.float32 or x.dtype == dtype:
        return x
    return _ToComputeFn.apply(x)


# =============================================================================== ViT pieces
class _LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, layer):
        y, mean, rstd = ops.layernorm_fwd(x.contiguous(), gamma.detach(), beta.detach(), layer._epsilon)
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        ctx.save_for_backward(x, mean, rstd)
        ctx.layer = layer
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        layer = ctx.layer
        for p in (layer.weight, layer.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dx = _ln_backward(dy.contiguous(), x, layer, mean, rstd, None)
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, None


def _ln_backward(dy, x, layer, mean, rstd, dres):
    """LayerNorm backward: the input gradient on the current stream; the fold of the per-block d-gamma / d-beta
    partials — a latency-bound launch nothing in the backward chain waits for (only the optimizer / the gradient
    reducer read its result, and both join the side stream first) — on the side stream when there is one."""
    if config.side_reductions() and streams.enabled(dy):
        dx, partials, fold = ops.layernorm_bwd(dy, x, layer.weight.detach(), mean, rstd, layer.weight.grad,
                                               layer.bias.grad, dres=dres, defer_params=True)
        streams.side_later(dy.device, fold, reads=(partials,))
        return dx
    return ops.layernorm_bwd(dy, x, layer.weight.detach(), mean, rstd, layer.weight.grad, layer.bias.grad, dres=dres)


class _LayerNormForkFn(Function):
    """(LN(x), x): the pre-norm residual fork `x + f(LN(x))`.  The second output is x itself, handed to
    the residual consumer (the GEMM epilogue of f's last Linear); in backward the gradient that comes
    back through it is added to the LayerNorm gradient INSIDE the LayerNorm backward kernel, so the fork
    costs no separate elementwise add."""

    @staticmethod
    def forward(ctx, x, gamma, beta, layer):
        x = x.contiguous()
        y, mean, rstd = ops.layernorm_fwd(x, gamma.detach(), beta.detach(), layer._epsilon)
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        ctx.save_for_backward(x, mean, rstd)
        ctx.layer = layer
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, dy, dres):
        x, mean, rstd = ctx.saved_tensors
        layer = ctx.layer
        for p in (layer.weight, layer.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        if dres is not None:
            dres = dres.contiguous()
            if dres.dtype != x.dtype:
                dres = dres.to(x.dtype)
        dx = _ln_backward(dy.contiguous(), x, layer, mean, rstd, dres)
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, None


class LayerNorm(Layer):
    """paddle.nn.LayerNorm over the last axis (biased variance), rows [M, C] in the compute dtype."""

    def fork(self, x):
        """-> (LN(x), x_for_the_residual_add); see _LayerNormForkFn."""
        return _LayerNormForkFn.apply(x, self.weight, self.bias, self)

    def __init__(self, normalized_shape, epsilon=1e-05, weight_attr=None, bias_attr=None, name=None):
        super().__init__()
        dev = config.get_device()
        n = normalized_shape if isinstance(normalized_shape, int) else normalized_shape[-1]
        self._epsilon = epsilon
        self.weight = tnn.Parameter(torch.ones(n, device=dev))
        self.bias = tnn.Parameter(torch.zeros(n, device=dev))
        self._rt = None

    def forward(self, x):
        return _LayerNormFn.apply(x, self.weight, self.bias, self)


class _DropPathAddFn(Function):
    """residual + keep_row[b] * (branch / keep_prob): the residual add of a block under stochastic depth
    (csrc/drop_path.hip).  Backward returns (dbranch, dy): the second goes back into LayerNorm.fork's ``dres`` exactly
    as the residual gradient of the fused GEMM epilogue does."""

    @staticmethod
    def forward(ctx, branch, residual, keep_row, keep_prob, B, T):
        ctx.save_for_backward(keep_row)
        ctx.args = (keep_prob, B, T)
        return ops.drop_path_add(branch.contiguous(), residual.contiguous(), keep_row, keep_prob, B, T)

    @staticmethod
    def backward(ctx, dy):
        (keep_row,) = ctx.saved_tensors
        keep_prob, B, T = ctx.args
        dy = dy.contiguous()
        return ops.drop_path_bwd(dy, keep_row, keep_prob, B, T), dy, None, None, None, None


def drop_path_add(branch, residual, keep_row, keep_prob, B, T):
    """keep_row: fp32 [B] on the device, 1 = sample kept, 0 = dropped (one row of the model's keep table)."""
    return _DropPathAddFn.apply(branch, residual, keep_row, keep_prob, B, T)


# =============================================================================== ConvNeXt pieces (csrc/dwconv.hip)
def _need_contiguous(who, **tensors):
    """A silent ``.contiguous()`` of a strided operand is a framework copy launch inside the step (foreign to a strict
    step plan): the ConvNeXt layers refuse such an operand by name instead."""
    for name, t in tensors.items():
        if not t.is_contiguous():
            raise ValueError('%s: %s must be contiguous (shape %s, strides %s)'
                             % (who, name, tuple(t.shape), tuple(t.stride())))


class _DepthwiseConvFn(Function):
    """Depthwise 7x7 over NHWC.  add_slot: the GradSlot into which the block's tail (layer_scale_add) puts the gradient
    of the residual fork `input + ...`; the data-gradient kernel adds it before its single rounding, so the fork costs
    no separate add launch.  dW and dbias are WRITTEN straight into the arena's gradient slices, on the side stream when
    there is one (they feed only the optimizer)."""

    @staticmethod
    def forward(ctx, x, weight, bias, layer, add_slot):
        _need_contiguous('DepthwiseConv2D', x=x)
        y = ops.dwconv7_fwd(x, weight.detach(), bias.detach())
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        if add_slot is not None and ctx.needs_input_grad[0]:
            add_slot.arm()
        ctx.save_for_backward(x)
        ctx.layer, ctx.add_slot = layer, add_slot
        ctx.side = streams.enabled(x)              # latched for the backward (see _ConvFn)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer = ctx.layer
        dy = dy.contiguous()
        for p in (layer.weight, layer.bias):
            if p.grad is None:
                p.grad = ops.zeros(*p.shape, dtype=p.dtype, device=p.device)      # (outside an arena; a library fill)
        dx = None
        if ctx.needs_input_grad[0]:
            add = ctx.add_slot.take() if ctx.add_slot is not None else None
            dx = ops.dwconv7_bwd_data(dy, layer.weight.detach(), add)
        dw, db = layer.weight.grad, layer.bias.grad
        if ctx.side:
            streams.side_later(dy.device, lambda: ops.dwconv7_bwd_weight_into(x, dy, dw, db), reads=(x, dy))
        else:
            ops.dwconv7_bwd_weight_into(x, dy, dw, db)
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, None, None


class DepthwiseConv2D(Layer):
    """paddle.nn.Conv2D(dim, dim, kernel_size=7, padding=3, groups=dim) over NHWC activations: parameters
    ``weight [dim, 1, 7, 7]`` and ``bias [dim]`` in the reference's layout, read by the kernels as they lie."""

    def __init__(self, dim, kernel_size=7, padding=3):
        super().__init__()
        if kernel_size != 7:
            raise NotImplementedError('DepthwiseConv2D: kernel_size %r (the HIP kernels are 7x7)' % (kernel_size,))
        if padding != 3:
            raise NotImplementedError('DepthwiseConv2D: padding %r (the HIP kernels pad by 3)' % (padding,))
        if dim <= 0 or dim % 8:
            raise NotImplementedError('DepthwiseConv2D: dim %r is not a positive multiple of 8' % (dim,))
        dev = config.get_device()
        self.dim = dim
        self.weight = tnn.Parameter(torch.empty(dim, 1, 7, 7, device=dev))
        self.bias = tnn.Parameter(torch.zeros(dim, device=dev))
        self._rt = None

    def forward(self, x, add_slot=None):
        """x: [N, H, W, dim] in the compute dtype."""
        return _DepthwiseConvFn.apply(x, self.weight, self.bias, self, add_slot)


# =============================================================================== ConvMAE pieces (csrc/convmae.hip)
class _MaskedDepthwiseConvFn(Function):
    """Depthwise 5x5 over NHWC of `keep * x`, keep = 1 - mask expanded from the patch grid by address arithmetic (no
    map-sized mask tensor).  No add_slot: a CBlock's residual forks before norm1, not at the convolution.  dW and dbias
    are WRITTEN straight into the parameters' gradients, on the side stream when there is one."""

    @staticmethod
    def forward(ctx, x, weight, bias, layer, mask, grid):
        _need_contiguous('MaskedDepthwiseConv2D', x=x)
        y = ops.dwconv5_masked_fwd(x, weight.detach(), bias.detach(), mask, grid)
        if layer._rt is not None and any(ctx.needs_input_grad):
            layer._rt.arena.expect_grad(layer._rt.indices)
        ctx.save_for_backward(x)
        ctx.layer, ctx.mask, ctx.grid = layer, mask, grid
        ctx.side = streams.enabled(x)              # latched for the backward (see _ConvFn)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer, mask, grid = ctx.layer, ctx.mask, ctx.grid
        dy = dy.contiguous()
        for p in (layer.weight, layer.bias):
            if p.grad is None:
                p.grad = ops.zeros(*p.shape, dtype=p.dtype, device=p.device)      # (outside an arena; a library fill)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.dwconv5_masked_bwd_data(dy, layer.weight.detach(), mask, grid)
        dw, db = layer.weight.grad, layer.bias.grad
        reads = (x, dy) if mask is None else (x, dy, mask)
        if ctx.side:
            streams.side_later(dy.device, lambda: ops.dwconv5_masked_bwd_weight_into(x, dy, dw, db, mask, grid),
                               reads=reads)
        else:
            ops.dwconv5_masked_bwd_weight_into(x, dy, dw, db, mask, grid)
        if layer._rt is not None:
            layer._rt.arena.grad_ready(layer._rt.indices)
        return dx, None, None, None, None, None


class MaskedDepthwiseConv2D(Layer):
    """paddle.nn.Conv2D(dim, dim, kernel_size=5, padding=2, groups=dim) over NHWC activations, applied to ``mask * x``
    as a ConvMAE CBlock does (conv_vit.py:82-99): parameters ``weight [dim, 1, 5, 5]`` and ``bias [dim]`` in the
    reference's layout, read by the kernels as they lie."""

    def __init__(self, dim, kernel_size=5, padding=2):
        super().__init__()
        if kernel_size != 5:
            raise NotImplementedError('MaskedDepthwiseConv2D: kernel_size %r (the HIP kernels are 5x5)' % (kernel_size,))
        if padding != 2:
            raise NotImplementedError('MaskedDepthwiseConv2D: padding %r (the HIP kernels pad by 2)' % (padding,))
        if dim <= 0 or dim % 8:
            raise NotImplementedError('MaskedDepthwiseConv2D: dim %r is not a positive multiple of 8' % (dim,))
        dev = config.get_device()
        self.dim = dim
        self.weight = tnn.Parameter(torch.empty(dim, 1, 5, 5, device=dev))
        self.bias = tnn.Parameter(torch.zeros(dim, device=dev))
        self._rt = None

    def forward(self, x, mask=None, grid=None):
        """x: [N, H, W, dim] in the compute dtype.  mask: the fp32 table [N, Hm * Wm] of ops.mae_mask (1 = removed) with
        grid = (Hm, Wm), H / Hm == W / Wm an integer; None: no mask (the ConvViT path)."""
        if mask is not None:
            if grid is None:
                raise ValueError('MaskedDepthwiseConv2D: a mask needs its grid (Hm, Wm)')
            Hm, Wm = grid
            H, W = x.shape[1], x.shape[2]
            if Hm <= 0 or Wm <= 0 or H % Hm or W % Wm or H // Hm != W // Wm:
                raise ValueError('MaskedDepthwiseConv2D: a %d x %d map does not lie over a %d x %d mask grid by one '
                                 'integer factor' % (H, W, Hm, Wm))
            _need_contiguous('MaskedDepthwiseConv2D', mask=mask)
        return _MaskedDepthwiseConvFn.apply(x, self.weight, self.bias, self, mask, None if mask is None else tuple(grid))


class _PatchGatherFn(Function):
    """The kept patches of an NHWC map as GEMM rows [B*K, p*p*C]; the backward writes every pixel of dx."""

    @staticmethod
    def forward(ctx, x, ids_keep, ids_restore, grid, p):
        _need_contiguous('patch_gather', x=x)
        ctx.ids_restore, ctx.grid, ctx.p = ids_restore, grid, p
        ctx.B, ctx.K, ctx.C = x.shape[0], ids_keep.shape[1], x.shape[3]
        return ops.patch_gather_fwd(x, ids_keep, grid, p)

    @staticmethod
    def backward(ctx, dout):
        dx = ops.patch_gather_bwd(dout.contiguous(), ctx.ids_restore, ctx.B, ctx.K, ctx.grid, ctx.p, ctx.C)
        return dx, None, None, None, None


def patch_gather(x, ids_keep, ids_restore, grid, p):
    """x [B, Hm*p, Wm*p, C] -> rows [B*K, p*p*C] of the patches ids_keep [B, K] names, column order (ph, pw, c): the
    operand of a patch convolution's GEMM restricted to the kept patches."""
    return _PatchGatherFn.apply(x, ids_keep, ids_restore, tuple(grid), p)


class _TokensPosGatherAddFn(Function):
    """out[b, k] = x[b, k] + pos[ids_keep[b, k]] (no class row).  dx is dout; a learnable ``pos`` (conv_mae.py leaves
    ``pos_embed`` trainable) gets its gradient added into ``pos.grad``, the images in ascending order."""

    @staticmethod
    def forward(ctx, x, pos, ids_keep, ids_restore, B, L):
        learnable = isinstance(pos, tnn.Parameter) and pos.requires_grad
        ctx.ids_restore, ctx.dims = ids_restore, (B, L, ids_keep.shape[1])
        ctx.params = (pos,) if learnable else ()
        param_expect_grad(*ctx.params)
        return ops.tokens_pos_gather_add(x, pos.detach().view(-1, pos.shape[-1]), ids_keep, B, L, ids_keep.shape[1])

    @staticmethod
    def backward(ctx, dout):
        B, L, K = ctx.dims
        dout = dout.contiguous()
        for pos in ctx.params:
            if pos.grad is None:
                pos.grad = torch.zeros_like(pos)
            ops.tokens_pos_gather_add_bwd_into(dout, ctx.ids_restore, pos.grad.view(-1, pos.shape[-1]), B, L, K)
        param_grad_ready(*ctx.params)
        return dout, None, None, None, None, None


def tokens_pos_gather_add(x, pos, ids_keep, ids_restore, B, L):
    """x [B*K, D] + the rows of pos [1, L, D] (a buffer or a learnable table) that ids_keep [B, K] names."""
    return _TokensPosGatherAddFn.apply(x, pos, ids_keep, ids_restore, B, L)


class _TokensUnshuffleFn(Function):
    """Decoder input without a class row: kept tokens back at their positions, the mask token elsewhere, + pos (a fixed
    table).  The mask token's gradient is added into ``mask_token.grad`` (as _UnshuffleFn of the MAE backbone does)."""

    @staticmethod
    def forward(ctx, x, mask_token, pos, ids_keep, ids_restore, B):
        ctx.ids = (ids_keep, ids_restore)
        ctx.tok, ctx.B = mask_token, B
        param_expect_grad(mask_token)
        return ops.tokens_unshuffle(x, mask_token.detach().view(-1), pos.detach().view(-1, pos.shape[-1]), ids_restore,
                                    B, ids_keep.shape[1])

    @staticmethod
    def backward(ctx, dout):
        ids_keep, ids_restore = ctx.ids
        tok = ctx.tok
        if tok.grad is None:
            tok.grad = torch.zeros_like(tok)
        dx = ops.tokens_unshuffle_bwd(dout.contiguous(), ids_keep, ids_restore, tok.grad.view(-1), ctx.B)
        param_grad_ready(tok)
        return dx, None, None, None, None, None


def tokens_unshuffle(x, mask_token, pos, ids_keep, ids_restore, B):
    """x [B*K, D] -> [B*L, D]."""
    return _TokensUnshuffleFn.apply(x, mask_token, pos, ids_keep, ids_restore, B)


class _TokensMAELossFn(Function):
    """MAE's masked-patch loss on prediction rows [B*L, p*p*3] without class rows (loss/mae.py has the form with)."""

    @staticmethod
    def forward(ctx, pred, imgs, mask, p, norm_pix, denom):
        ctx.save_for_backward(pred, imgs, mask)
        ctx.args = (p, norm_pix, denom)
        return ops.tokens_mae_loss_fwd(imgs, pred, mask, p, norm_pix, denom)

    @staticmethod
    def backward(ctx, gloss):
        pred, imgs, mask = ctx.saved_tensors
        p, norm_pix, denom = ctx.args
        return ops.tokens_mae_loss_bwd(imgs, pred, mask, gloss.contiguous().float(), p, norm_pix, denom), None, None, \
            None, None, None


def tokens_masked_patch_loss(pred_rows, imgs, mask, patch_size, norm_pix_loss, denom):
    """pred_rows fp32 [B*L, p*p*3], imgs fp32 [B, 3, H, W], mask [B, L] (1 = removed), denom = mask.sum() as the host
    knows it."""
    return _TokensMAELossFn.apply(pred_rows, imgs.contiguous().float(), mask, int(patch_size), bool(norm_pix_loss),
                                  float(denom))


class _PatchConvFn(Function):
    """Biased kernel = stride convolution over NHWC on the implicit-GEMM kernel: the bias is the epilogue's ``shift``,
    the data gradient goes through plan.dgrad_plan (stride 2 splits into residue classes), dW through wgrad_desc and
    the bias gradient is the column sum of dy; both parameter gradients are ACCUMULATED, as Linear's are, on the side
    stream when there is one."""

    @staticmethod
    def forward(ctx, x, weight, bias, layer):
        _need_contiguous('PatchConv2D', x=x)
        rt = _need_rt(layer)
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
        pl = layer._plan(N, H, W)
        y = torch.empty(N, pl.fd.OP, pl.fd.OQ, layer.geom.cout, dtype=x.dtype, device=x.device)
        ops.conv_igemm(pl.fd, x, rt.w_fwd, y, shift=bias.detach())
        if any(ctx.needs_input_grad):
            rt.arena.expect_grad(rt.indices)
        ctx.save_for_backward(x)
        ctx.layer, ctx.pl = layer, pl
        ctx.side = streams.enabled(x)              # latched for the backward (see _ConvFn)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer, pl = ctx.layer, ctx.pl
        rt, g = layer._rt, layer.geom
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            alloc = ops.zeros if pl.dgrad_zero else torch.empty
            dx = alloc(x.shape[0], x.shape[1], x.shape[2], g.cin, dtype=dy.dtype, device=dy.device)
            for d in pl.dds:
                ops.conv_igemm(d, dy, rt.w_dgrad[id(d.pack)], dx)
        rows = dy.view(-1, g.cout)
        bias_grad = layer.bias.grad

        def param_grads():
            ops.conv_wgrad(pl.wd, x, rows, rt.dw)
            ops.colsum_into(rows, bias_grad, accumulate=True)
        if ctx.side:
            streams.side_later(dy.device, param_grads, reads=(x, dy))
        else:
            param_grads()
        rt.arena.grad_ready(rt.indices)
        return dx, None, None, None


class PatchConv2D(Layer):
    """paddle.nn.Conv2D(cin, cout, kernel_size=k, stride=k) WITH bias over NHWC activations (ConvNeXt's 2x2/2 downsample
    layers, convnext.py:140-141).  ``weight`` is logically [cout, cin, k, k] (the reference's layout) and physically
    [cout][k][k][cin] in the arena, as Conv2D's.  Lives in an EncoderArena; ``Conv2D`` itself stays bias-free."""
    krsc_weight = True
    is_stem = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=None):
        super().__init__()
        stride = kernel_size if stride is None else stride
        if stride != kernel_size:
            raise NotImplementedError('PatchConv2D: stride %r != kernel_size %r (a patch convolution has kernel = stride)'
                                      % (stride, kernel_size))
        if in_channels % 8 or out_channels % 8:
            raise NotImplementedError('PatchConv2D: channels (%d -> %d) must be multiples of 8'
                                      % (in_channels, out_channels))
        dev = config.get_device()
        self.geom = P.ConvGeom(in_channels, out_channels, kernel_size, stride, 0)
        self.weight = tnn.Parameter(torch.empty(out_channels, in_channels, kernel_size, kernel_size, device=dev))
        self.bias = tnn.Parameter(torch.zeros(out_channels, device=dev))
        self._rt = None
        self._plans = {}

    def _plan(self, N, H, W):
        key = (N, H, W)
        pl = self._plans.get(key)
        if pl is None:
            rt = _need_rt(self)
            g = self.geom
            if H % g.k or W % g.k:
                raise NotImplementedError('PatchConv2D: input %d x %d is not a multiple of the patch %d' % (H, W, g.k))
            dds, skipped = ([], False)
            if rt.dgrad_packs is not None:
                dds, skipped = P.dgrad_plan(g, N, H, W, packs=rt.dgrad_packs)
            pl = SimpleNamespace(fd=P.fwd_desc(g, N, H, W), wd=P.wgrad_desc(g, N, H, W), dds=dds, dgrad_zero=skipped)
            self._plans[key] = pl
        return pl

    def forward(self, x):
        """x: [N, H, W, cin] in the compute dtype -> [N, H / k, W / k, cout]."""
        return _PatchConvFn.apply(x, self.weight, self.bias, self)


class _LayerScaleAddFn(Function):
    """residual + keep_row[b] * ((gamma * branch) / keep_prob): the tail of a ConvNeXt block (convnext.py:100-102).
    Backward: dbranch and dgamma (WRITTEN into gamma.grad) from one launch pair; the residual's gradient is dy itself:
    returned to autograd, or put into res_slot for the depthwise convolution's data gradient to add."""

    @staticmethod
    def forward(ctx, branch, residual, gamma, keep_row, keep_prob, B, T, res_slot):
        _need_contiguous('layer_scale_add', branch=branch, residual=residual)
        ctx.save_for_backward(branch, keep_row)
        ctx.gamma, ctx.args, ctx.res_slot = gamma, (keep_prob, B, T), res_slot
        return ops.layer_scale_add_fwd(branch, residual, gamma.detach(), keep_row, keep_prob, B, T)

    @staticmethod
    def backward(ctx, dy):
        branch, keep_row = ctx.saved_tensors
        gamma, (keep_prob, B, T) = ctx.gamma, ctx.args
        dy = dy.contiguous()
        if gamma.grad is None:
            gamma.grad = ops.zeros(*gamma.shape, dtype=gamma.dtype, device=gamma.device)
        dbranch = ops.layer_scale_add_bwd_into(dy, branch, gamma.detach(), keep_row, keep_prob, B, T, gamma.grad)
        param_grad_ready(gamma)
        dres = dy
        if ctx.res_slot is not None and ctx.res_slot.armed:
            ctx.res_slot.put(dy)
            dres = None
        return dbranch, dres, None, None, None, None, None, None


def layer_scale_add(branch, residual, gamma, keep_row, keep_prob, B, T, res_slot=None):
    """branch, residual: rows [B*T, C]; gamma: fp32 [C] parameter; keep_row: fp32 [B] on the device (one row of the
    model's keep table) or None (rate 0, evaluation)."""
    param_expect_grad(gamma)
    return _LayerScaleAddFn.apply(branch, residual, gamma, keep_row, keep_prob, B, T, res_slot)


class DropoutState:
    """What the dropout sites of ONE model share (csrc/dropout.hip): the rate as (thr, factor), the Philox key, the
    step counter in device memory and the ordinal of the current training pass on the host.

    ``begin_pass`` — once at the head of every training-mode forward — advances the device counter (one launch) and the
    ordinal.  Every site of that pass, forward and backward, then reads the same counter value, so the backward
    recomputes the forward's masks.  An autograd node remembers the ordinal it was made under; a backward under
    another ordinal (two training forwards before a backward) would draw different masks and raises instead."""

    def __init__(self, p, seed=0, step=0):
        self.p = float(p)
        self.thr, self.factor = ops.dropout_params(p)
        self.ordinal = 0
        self._step = None
        self.set_seed(seed, step)

    def set_seed(self, seed, step=0):
        self.seed = int(seed) & ((1 << 64) - 1)
        self.step0 = int(step) & ((1 << 64) - 1)
        if self._step is not None:
            self._step.fill_(self.step0 - (1 << 64) if self.step0 >= 1 << 63 else self.step0)

    def step(self):
        """The counter's value (reads the device: synchronises)."""
        return self.step0 if self._step is None else int(self._step.item()) & ((1 << 64) - 1)

    def begin_pass(self, device):
        if self._step is None:
            self._step = torch.zeros(1, dtype=torch.int64, device=device)
            self.set_seed(self.seed, self.step0)
        ops.dropout_advance(self._step)
        self.ordinal += 1

    def args(self, site):
        if self._step is None:
            raise RuntimeError('a dropout site ran before DropoutState.begin_pass: the step counter does not exist yet')
        return self.thr, self.factor, self.seed, self._step, int(site)

    def check(self, ordinal):
        if ordinal != self.ordinal:
            raise RuntimeError('dropout backward of training pass %d while the model is in pass %d: the step counter '
                               'has moved, the masks would differ from the forward\'s (run each backward before the '
                               'next training forward)' % (ordinal, self.ordinal))


def process_rank():
    """The rank that the seeds of stochastic depth and dropout are offset by: data-parallel ranks draw different masks."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.environ.get('RANK', 0))


class DropPathState:
    """The stochastic-depth state of ONE model (csrc/drop_path.hip): the keep table, its row layout, the Philox key and
    the step counter in device memory.

    ``blocks`` are the blocks that own rows of the table, in row order; each owns ``rows_per_block`` consecutive rows
    (1: the block's one residual; 2: its attention residual, then its MLP residual) and ``keep_probs`` — one float per
    row — repeats the block's ``keep_prob`` that often.  ``keep`` — once at the head of every forward — returns the
    table [len(keep_probs), B] of this pass: one ``passl_hip_drop_path_draw`` launch fills it from (seed, counter) and
    advances the counter on the device, so a replayed step plan or a captured graph draws a fresh table at every
    replay.  ``rows`` hands a block its rows of that table.

    A plain object, on purpose: nothing of it is in ``state_dict()`` or broadcast by ``param_sync``.  The counter, the
    keep-probability vector and one table per batch size are allocated at the first draw and never again (a recorded
    plan holds their addresses); ``set_seed`` refills the counter in place.  The constructor draws from no generator:
    the model seeds it from torch's global CPU generator plus the process rank, so ``torch.manual_seed(seed + rank)``
    reproduces a run and data-parallel ranks draw different masks.  A resumed run restarts the counter at 0."""

    def __init__(self, keep_probs, seed=0, step=0):
        self.keep_probs = [float(p) for p in keep_probs]
        self.blocks, self._rows = [], {}
        self.draws = 0                                    # tables drawn (host counter)
        self._dp_tables = {}                              # batch size -> keep table [len(keep_probs), B]
        self._dp_keep_prob = self._dp_step = None         # device state, made at the first draw
        self.set_seed(seed, step)

    @classmethod
    def for_blocks(cls, blocks, rows_per_block, seed=0, step=0):
        self = cls([blk.keep_prob for blk in blocks for _ in range(rows_per_block)], seed, step)
        self.blocks = list(blocks)
        for k, blk in enumerate(self.blocks):
            self._rows[blk] = k if rows_per_block == 1 else slice(rows_per_block * k, rows_per_block * (k + 1))
        return self

    def set_seed(self, seed, step=0):
        """Key of the Philox draw and the value of the step counter (the next draw uses it)."""
        self.seed = int(seed) & ((1 << 64) - 1)
        self.step0 = int(step)
        if self._dp_step is not None:
            self._dp_step.fill_(self.step0 - (1 << 64) if self.step0 >= 1 << 63 else self.step0)

    def step(self):
        """The counter's value = ``step`` of set_seed plus the draws since (reads the device: synchronises)."""
        return self.step0 if self._dp_step is None else int(self._dp_step.item()) & ((1 << 64) - 1)

    def table(self, B):
        """The table that the last draw of batch size B filled, or None."""
        return self._dp_tables.get(B)

    def keep(self, B, device, given=None):
        """-> the keep table of one forward pass: ``given`` (an injected table; no draw), or a fresh draw."""
        shape = (len(self.keep_probs), B)
        if given is not None:
            if tuple(given.shape) != shape:
                raise ValueError('drop_path_keep must be [%d, %d], got %s' % (shape + (tuple(given.shape),)))
            return given.to(device=device, dtype=torch.float32).contiguous()
        if self._dp_step is None:
            self._dp_keep_prob = torch.tensor(self.keep_probs, dtype=torch.float32, device=device)
            self._dp_step = torch.zeros(1, dtype=torch.int64, device=device)
            self.set_seed(self.seed, self.step0)
        keep = self._dp_tables.get(B)
        if keep is None:
            keep = self._dp_tables[B] = torch.empty(shape, dtype=torch.float32, device=device)
        self.draws += 1
        return ops.drop_path_draw(keep, self._dp_keep_prob, self.seed, self._dp_step)

    def rows(self, keep, blk):
        """-> the rows of the table ``keep`` that ``blk`` owns ([B] with one row per block, else [rows, B]), or None."""
        r = self._rows.get(blk)
        return None if r is None else keep[r]


class DropPathModel:
    """Mixin: the stochastic-depth surface of a model over ``self._drop_path``, a DropPathState, or None when nothing
    can drop (rate 0).  The model's constructor calls ``_seed_drop_path`` where its seed is drawn."""

    _drop_path = None

    def _seed_drop_path(self, blocks, rows_per_block):
        """``blocks``: those that own rows of the keep table.  With any, ONE draw from torch's global CPU generator."""
        blocks = list(blocks)
        if blocks:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            self._drop_path = DropPathState.for_blocks(blocks, rows_per_block, seed + process_rank())

    def set_drop_path_seed(self, seed, step=0):
        """Key of the Philox draw and the value of the device step counter (the next training forward uses it)."""
        if self._drop_path is not None:
            self._drop_path.set_seed(seed, step)

    def drop_path_step(self):
        """The step counter = the number of draws since set_drop_path_seed (reads the device: synchronises)."""
        return 0 if self._drop_path is None else self._drop_path.step()

    def drop_path_table(self, B):
        """The keep table the last training forward of batch size B used (None before the first)."""
        return None if self._drop_path is None else self._drop_path.table(B)

    @property
    def drop_path_draws(self):
        """Training forwards that drew a table (host counter)."""
        return 0 if self._drop_path is None else self._drop_path.draws

    def _drop_path_keep(self, B, device, given=None):
        """-> the keep table of this forward pass, or None when nothing can drop (evaluation mode, rate 0)."""
        if not (self.training and self._drop_path is not None):
            if given is not None:
                raise ValueError('drop_path_keep= needs a model in training mode built with drop_path_rate > 0')
            return None
        return self._drop_path.keep(B, device, given)

    def _drop_path_rows(self, keep, blk):
        """-> ``blk``'s rows of this pass's table, or None (no table, or a block that cannot drop)."""
        return None if keep is None else self._drop_path.rows(keep, blk)


class _DropoutFn(Function):
    """mask * (x * factor); the backward is the same launch on dy."""

    @staticmethod
    def forward(ctx, x, state, site):
        ctx.state, ctx.site, ctx.ordinal = state, site, state.ordinal
        return ops.dropout(x.contiguous(), *state.args(site))

    @staticmethod
    def backward(ctx, dy):
        ctx.state.check(ctx.ordinal)
        return ops.dropout(dy.contiguous(), *ctx.state.args(ctx.site)), None, None


class _DropoutAddFn(Function):
    """residual + mask * (branch * factor): the residual add of a block whose branch ends in a dropout.  Backward
    returns (mask * (dy * factor), dy): the second goes back into LayerNorm.fork's ``dres`` as _DropPathAddFn's does."""

    @staticmethod
    def forward(ctx, branch, residual, state, site):
        ctx.state, ctx.site, ctx.ordinal = state, site, state.ordinal
        return ops.dropout_add(branch.contiguous(), residual.contiguous(), *state.args(site))

    @staticmethod
    def backward(ctx, dy):
        ctx.state.check(ctx.ordinal)
        dy = dy.contiguous()
        return ops.dropout(dy, *ctx.state.args(ctx.site)), dy, None, None


class _GeluDropoutFn(Function):
    """mask * (gelu(x) * factor) in the GELU launch; backward (mask * (dy * factor)) * gelu'(x) in the GELU backward's."""

    @staticmethod
    def forward(ctx, x, state, site):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.state, ctx.site, ctx.ordinal = state, site, state.ordinal
        return ops.gelu_dropout_fwd(x, *state.args(site))

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        ctx.state.check(ctx.ordinal)
        return ops.gelu_dropout_bwd(dy.contiguous(), x, *ctx.state.args(ctx.site)), None, None


def dropout(x, state, site):
    return _DropoutFn.apply(x, state, site)


def dropout_add(branch, residual, state, site):
    return _DropoutAddFn.apply(branch, residual, state, site)


def gelu_dropout(x, state, site):
    return _GeluDropoutFn.apply(x, state, site)


class Dropout(Layer):
    """paddle.nn.Dropout(p) in its default ``upscale_in_train`` mode [Paddle-semantics]: training
    ``kept ? x / (1 - p) : 0``, evaluation the identity.  The mask is a function of (seed, step, site, position)
    (csrc/dropout.hip); the owning model binds the layer to its DropoutState and a site number."""

    def __init__(self, p=0.5, axis=None, mode='upscale_in_train', name=None):
        super().__init__()
        if mode != 'upscale_in_train':
            raise NotImplementedError("Dropout(mode=%r): only 'upscale_in_train' is built" % (mode,))
        if axis is not None:
            raise NotImplementedError('Dropout(axis=...) is not built')
        ops.dropout_params(p)                              # refuses a rate outside [0, 1)
        self.p = float(p)
        self.state = self.site = None

    def bind(self, state, site):
        self.state, self.site = state, int(site)
        return self

    def forward(self, x):
        if not (self.training and self.p > 0.):
            return x
        if self.state is None:
            raise RuntimeError('Dropout(p=%g) in training mode is not bound to a DropoutState / site' % self.p)
        return dropout(x, self.state, self.site)


class _UnaryFn(Function):
    """A streaming activation: fwd(x) -> y and bwd(dy, x) -> dx are the op's two functions of ops."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        x = x.contiguous()              # saved as the kernels read it: dy arrives in the layout of y
        ctx.save_for_backward(x)
        ctx.bwd = bwd
        return fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return ctx.bwd(dy.contiguous(), x), None, None


def gelu(x):
    return _UnaryFn.apply(x, ops.gelu_fwd, ops.gelu_bwd)


class GELU(Layer):
    def forward(self, x):
        return gelu(x)


class Tanh(Layer):
    def forward(self, x):
        return _UnaryFn.apply(x, ops.tanh_fwd, ops.tanh_bwd)


class _AttentionFn(Function):
    """softmax(q k^T * scale) v per (image, head) on the fused qkv projection [B*T, 3*H*d]."""

    @staticmethod
    def forward(ctx, qkv, B, T, H, DH, scale, causal):
        out, lse = ops.attention_fwd(qkv.contiguous(), B, T, H, DH, scale, causal)
        ctx.save_for_backward(qkv, out, lse)
        ctx.dims = (B, T, H, DH, scale, causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, H, DH, scale, causal = ctx.dims
        return ops.attention_bwd(qkv, out, dout.contiguous(), lse, B, T, H, DH, scale, causal), None, None, \
            None, None, None, None


class _AttentionTiledFn(Function):
    """_AttentionFn beyond ops.ATTENTION_MAX_TOKENS: the key-tiled kernels (csrc/attention_tiled.hip), no causal flag."""

    @staticmethod
    def forward(ctx, qkv, B, T, H, DH, scale):
        out, lse = ops.attention_tiled_fwd(qkv.contiguous(), B, T, H, DH, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.dims = (B, T, H, DH, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, T, H, DH, scale = ctx.dims
        return ops.attention_tiled_bwd(qkv, out, dout.contiguous(), lse, B, T, H, DH, scale), None, None, None, None, \
            None


def param_expect_grad(*params):
    """Called from the FORWARD of a custom Function that will report ``param_grad_ready`` for these raw arena parameters
    from its backward: a parameter used by several forward nodes of one step (a trunk run once per view) is complete —
    ready for its all-reduce bucket — only after the last contribution (EncoderArena.expect_grad)."""
    if not torch.is_grad_enabled():
        return
    for p in params:
        a = getattr(p, '_passl_arena', None)
        if a is not None and p.requires_grad:
            a.expect_grad([p._passl_index])


def param_grad_ready(*params):
    """Report raw arena parameters as reduced-ready from a custom backward (no-op outside an arena)."""
    for p in params:
        a = getattr(p, '_passl_arena', None)
        if a is not None:
            a.param_grad_ready(p)


def attention(qkv, B, T, H, DH, scale, causal=False, key_bias=None):
    """``key_bias``: fp32 [B, T] added to every score of its key before the softmax (proportional attention of token
    merging, log of the token sizes).  Forward only, as the reference uses it (tome.py:279-280).
    Beyond ``ops.ATTENTION_MAX_TOKENS`` tokens the key-tiled kernels take over; they have neither mask nor bias."""
    if T > ops.ATTENTION_MAX_TOKENS:
        if causal or key_bias is not None:
            raise NotImplementedError('attention(causal / key_bias) beyond %d tokens is not built: the key-tiled '
                                      'kernels have neither' % ops.ATTENTION_MAX_TOKENS)
        return _AttentionTiledFn.apply(qkv, B, T, H, DH, float(scale))
    if key_bias is None:
        return _AttentionFn.apply(qkv, B, T, H, DH, float(scale), bool(causal))
    if causal:
        raise NotImplementedError('attention(key_bias=...) with the causal mask is not built')
    if torch.is_grad_enabled() and qkv.requires_grad:
        raise NotImplementedError('attention(key_bias=...) has no backward: proportional attention is for evaluation '
                                  '(run it under torch.no_grad())')
    return ops.attention_fwd_keybias(qkv.contiguous(), key_bias, B, T, H, DH, float(scale))[0]


class _PrefixTokensFn(Function):
    """rows[b] = [prefix rows | x[b]] + pos with one or two learnable prefix rows and a learnable position table
    (csrc/deit_tokens.hip).  Backward: dx is a copy, each dprefix the batch sum of its row of dout, dpos the column sum."""

    @staticmethod
    def forward(ctx, x, pos, B, L, *prefixes):
        ctx.params = tuple(prefixes) + (pos,)
        ctx.dims = (B, L)
        param_expect_grad(*ctx.params)
        return ops.prefix_tokens_fwd(x.contiguous(), [p.detach().view(-1) for p in prefixes],
                                     pos.detach().view(-1, pos.shape[-1]), B, L)

    @staticmethod
    def backward(ctx, dout):
        B, L = ctx.dims
        for p in ctx.params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        dout = dout.contiguous()
        dx = ops.prefix_tokens_bwd(dout, [p.grad.view(-1) for p in ctx.params[:-1]], B, L)
        ops.colsum_into(dout.view(B, -1), ctx.params[-1].grad.view(-1), accumulate=True)    # dpos[t] += sum_b dout[b, t]
        param_grad_ready(*ctx.params)
        return (dx, None, None, None) + (None,) * (len(ctx.params) - 1)


def prefix_tokens(x, prefixes, pos, B, L):
    """x [B*L, C] -> [B*(len(prefixes) + L), C]: concat(*prefixes, x) + pos (deit.py:242-246)."""
    return _PrefixTokensFn.apply(x, pos, B, L, *prefixes)


class _Mean2Fn(Function):
    """(a + b) / 2 on fp32 logits in one launch; both inputs receive dy / 2."""

    @staticmethod
    def forward(ctx, a, b):
        return ops.mean2(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, dy):
        g = ops.mean2(dy.contiguous())
        return g, g


def mean2(a, b):
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape:
        raise ValueError('mean2 takes two fp32 tensors of one shape')
    return _Mean2Fn.apply(a, b)


class _ToMeMergeFn(Function):
    """merge_wavg over a matching: y[row] = sum of size[t] x[t] over the tokens with dest[t] = row, over the sum of
    their sizes (csrc/tome.hip).  The matching and the sizes carry no gradient; dx is a gather of dy."""

    @staticmethod
    def forward(ctx, x, size, dest, B, T, r, want_log):
        _need_contiguous('tome_merge', x=x)
        res = ops.tome_merge_fwd(x, size, dest, B, T, r, want_log=want_log)
        ctx.save_for_backward(dest, res[1], *(() if size is None else (size,)))
        ctx.dims = (B, T, r)
        ctx.mark_non_differentiable(*res[1:])
        ctx.set_materialize_grads(False)            # no zero tensor for the sizes' unused gradient (a framework launch)
        return res

    @staticmethod
    def backward(ctx, dy, *unused):
        dest, size_out, *size = ctx.saved_tensors
        B, T, r = ctx.dims
        return ops.tome_merge_bwd(dy.contiguous(), size[0] if size else None, size_out, dest, B, T, r), None, None, \
            None, None, None, None


def tome_merge(x, size, dest, B, T, r, want_log=False):
    """-> (y [B*(T-r), C], size_out fp32 [B, T-r]) and with ``want_log`` also log(size_out)."""
    return _ToMeMergeFn.apply(x, size, dest, B, T, r, bool(want_log))


class _WindowAttentionFn(Function):
    """Shifted-window attention with the relative-position bias (csrc/window_attention.hip) on the qkv projection of the
    unshifted, unpartitioned tokens.  Backward: dqkv, and dtable WRITTEN into table.grad."""

    @staticmethod
    def forward(ctx, qkv, table, B, Hp, Wp, ws, shift, nH, DH, scale):
        _need_contiguous('window_attention', qkv=qkv)
        out, lse = ops.window_attention_fwd(qkv, table.detach(), B, Hp, Wp, ws, shift, nH, DH, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.table, ctx.dims = table, (B, Hp, Wp, ws, shift, nH, DH, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        table = ctx.table
        from_arena = getattr(table, '_passl_arena', None) is not None
        dtable = table.grad if from_arena else None
        if dtable is None:
            dtable = ops.zeros(*table.shape, dtype=table.dtype, device=table.device)
            if from_arena:
                table.grad = dtable
        dqkv = ops.window_attention_bwd_into(qkv, table.detach(), out, dout.contiguous(), lse, dtable, *ctx.dims)
        if from_arena:
            param_grad_ready(table)
            return (dqkv,) + (None,) * 9
        return (dqkv, dtable) + (None,) * 8


def window_attention(qkv, table, B, Hp, Wp, ws, shift, nH, DH, scale):
    """qkv: rows [B*Hp*Wp, 3*nH*DH]; table: the fp32 [(2 ws - 1)^2, nH] relative_position_bias_table.  A table that is
    a parameter of an arena has its gradient written in place (as layer_scale_add's gamma); any other tensor gets it
    from autograd."""
    param_expect_grad(table)
    return _WindowAttentionFn.apply(qkv, table, B, Hp, Wp, ws, shift, nH, DH, float(scale))


class _TalkingHeadsAttentionFn(Function):
    """CaiT's talking-heads attention (csrc/cait_attention.hip) on the fused qkv projection [B*T, 3*H*48]: both Linears
    over the head axis run inside the kernel.  Backward: dqkv, and the four small gradients WRITTEN into the .grad of
    arena parameters (returned through autograd for any other tensor)."""

    @staticmethod
    def forward(ctx, qkv, wl, bl, ww, bw, B, T, H, DH, scale):
        _need_contiguous('talking_heads_attention', qkv=qkv)
        out, lse = ops.talking_heads_attention_fwd(qkv, wl.detach(), bl.detach(), ww.detach(), bw.detach(), B, T, H,
                                                   DH, scale)
        ctx.save_for_backward(qkv, lse)
        ctx.mix, ctx.dims = (wl, bl, ww, bw), (B, T, H, DH, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, lse = ctx.saved_tensors
        mix = ctx.mix
        from_arena = all(getattr(p, '_passl_arena', None) is not None for p in mix)
        grads = []
        for p in mix:
            g = p.grad if from_arena else None
            if g is None:
                g = ops.zeros(*p.shape, dtype=p.dtype, device=p.device)
                if from_arena:
                    p.grad = g
            grads.append(g)
        dqkv = ops.talking_heads_attention_bwd_into(qkv, *(p.detach() for p in mix), dout.contiguous(), lse, *grads,
                                                    *ctx.dims)
        if from_arena:
            param_grad_ready(*mix)
            return (dqkv,) + (None,) * 9
        return (dqkv,) + tuple(grads) + (None,) * 5


def talking_heads_attention(qkv, wl, bl, ww, bw, B, T, H, DH, scale):
    """qkv: rows [B*T, 3*H*DH]; wl, bl / ww, bw: the fp32 proj_l / proj_w weight [H, H] ([in, out]) and bias [H]."""
    param_expect_grad(wl, bl, ww, bw)
    return _TalkingHeadsAttentionFn.apply(qkv, wl, bl, ww, bw, B, T, H, DH, float(scale))


class _ClassAttentionFn(Function):
    """CaiT's class attention (csrc/cait_attention.hip): one query per (image, head), the projected class row."""

    @staticmethod
    def forward(ctx, q, k, v, B, T, H, DH, scale):
        _need_contiguous('class_attention', q=q, k=k, v=v)
        out, lse = ops.class_attention_fwd(q, k, v, B, T, H, DH, scale)
        ctx.save_for_backward(q, k, v, lse)
        ctx.dims = (B, T, H, DH, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, lse = ctx.saved_tensors
        return ops.class_attention_bwd(q, k, v, dout.contiguous(), lse, *ctx.dims) + (None,) * 5


def class_attention(q, k, v, B, T, H, DH, scale):
    """q: rows [B, H*DH]; k, v: rows [B*T, H*DH] -> [B, H*DH]."""
    return _ClassAttentionFn.apply(q, k, v, B, T, H, DH, float(scale))


class _CrossAttentionFn(Function):
    """CAE's cross-attention (csrc/cross_attention.hip): Tq queries against Tk keys, q / k / v three tensors."""

    @staticmethod
    def forward(ctx, q, k, v, B, Tq, Tk, H, DH, scale):
        _need_contiguous('cross_attention', q=q, k=k, v=v)
        out, lse = ops.cross_attention_fwd(q, k, v, B, Tq, Tk, H, DH, scale)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.dims = (B, Tq, Tk, H, DH, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        return ops.cross_attention_bwd(q, k, v, out, dout.contiguous(), lse, *ctx.dims) + (None,) * 6


def cross_attention(q, k, v, B, Tq, Tk, H, DH, scale):
    """q: rows [B*Tq, H*DH]; k, v: rows [B*Tk, H*DH] -> [B*Tq, H*DH]."""
    return _CrossAttentionFn.apply(q, k, v, B, Tq, Tk, H, DH, float(scale))


class _CAETokensAssembleFn(Function):
    """The regressor's operands from the visible and the masked rows and the fixed position table (csrc/cae.hip)."""

    @staticmethod
    def forward(ctx, xu, xm, pos, ids_vis, ids_msk, B, u0):
        _need_contiguous('cae_tokens_assemble', xu=xu, xm=xm)
        ctx.dims = (B, ids_vis.shape[1], ids_msk.shape[1], u0)
        return ops.cae_tokens_assemble(xu, xm, pos, ids_vis, ids_msk, B, u0=u0)

    @staticmethod
    def backward(ctx, dq_in, dk_in, dv_in):
        g = [None if t is None else t.contiguous() for t in (dq_in, dk_in, dv_in)]
        return ops.cae_tokens_assemble_bwd(g[0], g[1], g[2], *ctx.dims) + (None,) * 5


def cae_tokens_assemble(xu, xm, pos, ids_vis, ids_msk, B, u0=0):
    """xu [B*(u0+Nu), C] (the first u0 rows of every image are skipped), xm [B*Nm, C] ->
    (q_in [B*Nm, C], k_in [B*(Nu+Nm), C], v_in [B*(Nu+Nm), C])."""
    return _CAETokensAssembleFn.apply(xu, xm, pos, ids_vis, ids_msk, B, u0)


class _CAEPosAddFn(Function):
    """x_masked + pos[1 + ids_msk]: the same entry with q_in only; the gradient passes through unchanged."""

    @staticmethod
    def forward(ctx, xm, pos, ids_msk, B):
        _need_contiguous('cae_pos_add', xm=xm)
        return ops.cae_tokens_assemble(None, xm, pos, None, ids_msk, B, want_kv=False)[0]

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None, None


def cae_pos_add(xm, pos, ids_msk, B):
    return _CAEPosAddFn.apply(xm, pos, ids_msk, B)


class _MSEFn(Function):
    """F.mse_loss(pred.float(), target.float(), 'mean') with the target read from row t0 of every image; the target has
    no gradient."""

    @staticmethod
    def forward(ctx, pred, target, B, Tm, t0):
        _need_contiguous('mse_loss', pred=pred, target=target)
        ctx.save_for_backward(pred, target)
        ctx.dims = (B, Tm, t0)
        return ops.mse_fwd(pred, target, B, Tm, t0)

    @staticmethod
    def backward(ctx, gloss):
        pred, target = ctx.saved_tensors
        return ops.mse_bwd(pred, target, gloss.contiguous().float(), *ctx.dims), None, None, None, None


def mse_loss(pred, target, B, Tm, t0=0):
    """pred rows [B*Tm, C], target rows [B*(Tm + t0), C] -> fp32 [1]."""
    return _MSEFn.apply(pred, target.detach(), B, Tm, t0)


class _PosAddFn(Function):
    """rows [B*L, C] + pos_embed [1, L, C] (cait.py:354).  Backward: dx is dout; dpos += its column sums over the batch,
    straight into pos.grad."""

    @staticmethod
    def forward(ctx, x, pos, B, L):
        _need_contiguous('pos_add', x=x)
        ctx.pos, ctx.dims = pos, (B, L)
        param_expect_grad(pos)
        return ops.cait_pos_add(x, pos.detach(), B, L)

    @staticmethod
    def backward(ctx, dout):
        pos, (B, L) = ctx.pos, ctx.dims
        if pos.requires_grad:
            if pos.grad is None:
                pos.grad = ops.zeros(*pos.shape, dtype=pos.dtype, device=pos.device)
            ops.colsum_into(dout.contiguous().view(B, -1), pos.grad.view(-1), accumulate=True)
            param_grad_ready(pos)
        return dout, None, None, None


def pos_add(x, pos, B, L):
    return _PosAddFn.apply(x, pos, B, L)


class _ClsConcatFn(Function):
    """concat(c, x) along the token axis: rows [B*(L+1), C] whose row 0 of every image is the class row.  ``c`` is rows
    [B, C], or the fp32 ``cls_token`` parameter (cait.py:360: its expand is an address, its gradient the column sum of
    the class rows' gradient, added into cls_token.grad).  The patch rows x feed every token-only block: ``slot_in`` /
    ``slot_out`` chain their gradients through the split launches instead of an add of autograd's.  A block's backward
    runs before that of the block before it, so the LAST block has slot_out only and the FIRST slot_in only."""

    @staticmethod
    def forward(ctx, x, c, B, L, slot_in, slot_out):
        _need_contiguous('cls_concat', x=x, c=c)
        ctx.cls = c if isinstance(c, tnn.Parameter) else None
        if ctx.cls is not None:
            param_expect_grad(c)
            c = ops.cast_to(c.detach().view(1, -1), x.dtype)
        if slot_out is not None and ctx.needs_input_grad[0]:
            slot_out.arm()
        ctx.dims, ctx.slot_in, ctx.slot_out = (B, L), slot_in, slot_out
        return ops.cait_cls_concat(c, x, B, L)

    @staticmethod
    def backward(ctx, dout):
        B, L = ctx.dims
        add = ctx.slot_in.take() if (ctx.slot_in is not None and ctx.slot_in.armed) else None
        dc, dx = ops.cait_cls_split(dout.contiguous(), add, B, L)
        if ctx.cls is not None:
            cls = ctx.cls
            if cls.grad is None:
                cls.grad = ops.zeros(*cls.shape, dtype=cls.dtype, device=cls.device)
            ops.colsum_into(dc, cls.grad.view(-1), accumulate=True)
            param_grad_ready(cls)
            dc = None
        if ctx.slot_out is not None and ctx.slot_out.armed:
            ctx.slot_out.put(dx)
            dx = None
        return dx, dc, None, None, None, None


def cls_concat(x, c, B, L, slot_in=None, slot_out=None):
    return _ClsConcatFn.apply(x, c, B, L, slot_in, slot_out)


class _ForkFn(Function):
    """n aliases of rows x whose gradients are added by the library (residual + 1 * branch of csrc/drop_path.hip), not
    by autograd: a tensor with several consumers inside a step plan."""

    @staticmethod
    def forward(ctx, x, n, ones, B, T):
        ctx.save_for_backward(ones)
        ctx.dims = (B, T)
        return tuple(x.view(x.shape) for _ in range(n))

    @staticmethod
    def backward(ctx, *grads):
        (ones,) = ctx.saved_tensors
        B, T = ctx.dims
        acc = None
        for g in grads:
            if g is None:
                continue
            g = g.contiguous()
            acc = g if acc is None else ops.drop_path_add(g, acc, ones, 1.0, B, T)
        return acc, None, None, None, None


def fork(x, n, ones, B, T):
    """ones: fp32 [B] of 1 on the device."""
    return _ForkFn.apply(x, n, ones, B, T)


class _PatchMergeFn(Function):
    """PatchMerging's gather of four neighbours [B*H*W, C] -> [B*(H/2)*(W/2), 4C]; the backward is the inverse copy."""

    @staticmethod
    def forward(ctx, x, B, H, W):
        _need_contiguous('patch_merge', x=x)
        ctx.dims = (B, H, W)
        return ops.patch_merge(x, B, H, W)

    @staticmethod
    def backward(ctx, dy):
        return ops.patch_merge_bwd(dy.contiguous(), *ctx.dims), None, None, None


def patch_merge(x, B, H, W):
    return _PatchMergeFn.apply(x, B, H, W)


class QuickGELU(Layer):
    """x * sigmoid(1.702 x) (passl_v110/modeling/backbones/base_transformer.py:25-28)."""

    def forward(self, x):
        return _UnaryFn.apply(x, ops.quick_gelu_fwd, ops.quick_gelu_bwd)


class _GatherRowsFn(Function):
    """out[r] = x[idx[r]] for distinct row indices (class token / EOT token selection)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.save_for_backward(idx)
        ctx.rows = x.shape[0]
        return ops.gather_rows(x.contiguous(), idx)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        return ops.scatter_rows(dout.contiguous(), idx, ctx.rows), None


def gather_rows(x, idx):
    return _GatherRowsFn.apply(x, idx)


class _SplitRowsFn(Function):
    """x [M, C] -> (x[:n], x[n:]) as tensors of their own (two library copies); the backward writes both gradients
    into one [M, C] buffer.  A slice's own backward would be ATen launches inside the step."""

    @staticmethod
    def forward(ctx, x, n):
        x = x.contiguous()
        ctx.n, ctx.shape = n, x.shape
        return ops.clone(x[:n]), ops.clone(x[n:])

    @staticmethod
    def backward(ctx, d0, d1):
        dx = torch.empty(ctx.shape, dtype=(d0 if d0 is not None else d1).dtype, device=(d0 if d0 is not None else d1).device)
        for part, d in ((dx[:ctx.n], d0), (dx[ctx.n:], d1)):
            if d is None:
                ops.fill_zero(part)
            else:
                ops.copy_into(part, d.contiguous())
        return dx, None


def split_rows(x, n):
    return _SplitRowsFn.apply(x, n)


# =============================================================================== head pieces
class _L2NormFn(Function):
    @staticmethod
    def forward(ctx, x, eps):
        y, norm = ops.l2norm_fwd(x.contiguous(), eps)
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, norm = ctx.saved_tensors
        return ops.l2norm_bwd(dy.contiguous(), y, norm, torch.float32), None


def normalize(x, axis=1, epsilon=1e-12):
    """paddle.nn.functional.normalize(x, axis=1) for [N, D] fp32 rows."""
    assert x.dim() == 2 and axis in (1, -1)
    return _L2NormFn.apply(x, epsilon)


def infonce(q, k, queue, T):
    """Fused InfoNCE — lives in passl_amd/loss/moco.py (``passl.loss.moco``)."""
    from ..loss.moco import info_nce
    return info_nce(q, k, queue, T)


# =============================================================================== arena
class EncoderArena:
    """Flat fp32 storage for one encoder (see module docstring)."""

    ALIGN = 8   # elements; keeps every slot 32-byte aligned in fp32 and 16-byte aligned in bf16

    def __init__(self, module, trainable=True, dtype=None, exclude=(), exclude_params=()):
        """exclude: sub-layers whose own parameters / statistics live elsewhere (a frozen layer inside a trainable
        encoder gets a non-trainable arena of its own, e.g. MoCo-v3's patch embedding).  exclude_params: single
        parameters that stay ordinary tensors outside the arena (SimSiam's projector bias whose gradient is
        switched off, passl/models/simsiam.py:61)."""
        self.module = module
        skip = {id(m) for m in exclude}
        skip_p = {id(q) for q in exclude_params}
        self.trainable = trainable
        self.dtype = dtype or config.get_compute_dtype()
        self.reducer = None
        self._uses = {}          # parameter index -> forward uses of this step still waiting for their backward
        self.bn_affine = None
        params = []      # (owner, name, kind)
        seen = set()
        for mod in module.modules():
            if id(mod) in skip:
                continue
            for name, p in mod._parameters.items():
                if p is None or id(p) in seen or id(p) in skip_p:
                    continue
                seen.add(id(p))
                kind = 'conv' if ((isinstance(mod, Conv2D) or getattr(mod, 'krsc_weight', False))
                                  and name == 'weight') else \
                    ('linw' if isinstance(mod, Linear) and name == 'weight' else 'vec')
                params.append((mod, name, kind))
        stats = [(mod, n) for mod in module.modules() if isinstance(mod, _BatchNormBase) and id(mod) not in skip
                 for n in ('_mean', '_variance')]
        if not params:
            raise ValueError('EncoderArena over a module without parameters')
        if trainable and any(not m._parameters[n].requires_grad for m, n, _k in params):
            raise NotImplementedError(
                'a trainable EncoderArena holds only trainable parameters: frozen sub-layers (e.g. '
                'ResNet(frozen_stages >= 0)) belong in their own non-trainable arena — see '
                'modeling/architectures/clas.py; the pre-training architectures use frozen_stages -1')
        dev = params[0][0]._parameters[params[0][1]].device
        self.device = dev

        def aligned(n):
            return (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN

        off = 0
        self.param_slices = []   # (off, numel) per trainable parameter, registration order
        slots = []
        for mod, name, kind in params:
            n = mod._parameters[name].numel()
            slots.append((mod, name, kind, off, n))
            self.param_slices.append((off, n))
            off += aligned(n)
        self.n_train = off
        stat_slots = []
        for mod, name in stats:
            n = mod._buffers[name].numel()
            stat_slots.append((mod, name, off, n))
            off += aligned(n)
        self.total = off
        self.flat = torch.zeros(self.total, dtype=torch.float32, device=dev)
        self.grads = torch.zeros(self.n_train, dtype=torch.float32, device=dev) if trainable else None
        self.lp = torch.zeros(self.total, dtype=torch.bfloat16, device=dev) \
            if self.dtype == torch.bfloat16 else None
        self.packer = WeightPacker()
        owners = {}
        for index, (mod, name, kind, o, n) in enumerate(slots):
            old = mod._parameters[name].detach()
            seg = self.flat[o:o + n]
            if kind == 'conv':
                K, Cc, R, S = old.shape
                seg.view(K, R, S, Cc).copy_(old.permute(0, 2, 3, 1))
                view = seg.view(K, R, S, Cc).permute(0, 3, 1, 2)
                gview = self.grads[o:o + n].view(K, R, S, Cc).permute(0, 3, 1, 2) if trainable else None
            elif kind == 'linw':
                i, oo = old.shape
                seg.view(oo, i).copy_(old.t())
                view = seg.view(oo, i).t()
                gview = self.grads[o:o + n].view(oo, i).t() if trainable else None
            else:
                seg.copy_(old.reshape(-1))
                view = seg.view(old.shape)
                gview = self.grads[o:o + n].view(old.shape) if trainable else None
            p = tnn.Parameter(view, requires_grad=trainable)
            p._passl_arena = self
            p._passl_index = index          # position in param_slices (for param_grad_ready)
            if trainable:
                p.grad = gview
            mod._parameters[name] = p
            rt = owners.get(id(mod))
            if rt is None:
                rt = SimpleNamespace(arena=self, indices=[], dgrad_packs=None, w_dgrad={},
                                     bn_slice=None)
                owners[id(mod)] = rt
                mod._rt = rt
            rt.indices.append(index)
            if kind in ('conv', 'linw'):
                self._attach_gemm_layer(mod, rt, o, n)
        for mod, name, o, n in stat_slots:
            seg = self.flat[o:o + n]
            seg.copy_(mod._buffers[name])
            mod._buffers[name] = seg
        # index tensors for the one-shot inference-BN affine of all layers
        gi, bi, mi, vi, pos = [], [], [], [], 0
        slot_of = {(id(m), nm): (o, n) for m, nm, _k, o, n in slots}
        slot_of.update({(id(m), nm): (o, n) for m, nm, o, n in stat_slots})
        self._bn_eps = 1e-5
        for mod in module.modules():
            # (a BatchNorm without gamma / beta has no slot to fold from: it keeps the per-layer path)
            if isinstance(mod, _BatchNormBase) and mod.affine and id(mod) not in skip:
                Cc = mod.num_features
                for lst, nm in ((gi, 'weight'), (bi, 'bias'), (mi, '_mean'), (vi, '_variance')):
                    o, _ = slot_of[(id(mod), nm)]
                    lst.append(torch.arange(o, o + Cc))
                mod._rt.bn_slice = (pos, pos + Cc)
                pos += (Cc + 7) // 8 * 8          # keep every slice 32-byte aligned
                self._bn_eps = mod._epsilon
        self._bn_idx = None
        if gi:
            def cat_pad(lst):
                outs = []
                for t in lst:
                    padn = (-len(t)) % 8
                    outs.append(t)
                    if padn:
                        outs.append(t[:1].expand(padn))
                return torch.cat(outs).to(dev)
            self._bn_idx = tuple(cat_pad(lst) for lst in (gi, bi, mi, vi))
        self.packer.build(dev, self.dtype)
        # resolve packed-operand views now that the packer buffer exists
        for rt in owners.values():
            if getattr(rt, '_pending', None):
                rt._pending()
                rt._pending = None
        self._refresh_if_on_device()

    def _attach_gemm_layer(self, mod, rt, off, n):
        g = mod.geom
        rows = g.cout
        is_stem = getattr(mod, 'is_stem', False)
        rt.dw = self.grads[off:off + n].view(rows, -1) if self.trainable else None
        stem_pack = None
        if is_stem:
            stem_pack = P.stem_desc(g.cout, 1, 8, 8).pack
            self.packer.add(off, g.cout, g.k, g.k, g.cin, stem_pack)
        elif self.trainable and not getattr(mod, 'no_dgrad', False):
            rt.dgrad_packs = P.dgrad_packs(g)
            for pk in rt.dgrad_packs.values():
                self.packer.add(off, g.cout, g.k, g.k, g.cin, pk)

        def resolve():
            if is_stem:
                rt.w_fwd = self.packer.view(stem_pack, g.cout)
            elif self.lp is not None:
                rt.w_fwd = self.lp[off:off + n].view(rows, -1)
            else:
                rt.w_fwd = self.flat[off:off + n].view(rows, -1)
            if rt.dgrad_packs:
                rt.w_dgrad = {id(pk): self.packer.view(pk, g.cin) for pk in rt.dgrad_packs.values()}
        rt._pending = resolve

    # ---- per-step maintenance
    @torch.no_grad()
    def refresh(self):
        """Recompute the compute-dtype operand copies from the fp32 master weights."""
        if self.lp is not None:
            ops.cast_bf16(self.flat[:self.n_train], self.lp[:self.n_train])
        self.packer.run(self.flat)

    @torch.no_grad()
    def ema_from(self, other, m):
        """self = self*m + other*(1-m) over parameters AND BN statistics (one launch), then refresh
        the stem pack and the fused-BN affine.  moco.py:82-90 semantics (SURVEY §3.1 note A)."""
        ops.ema_update(self.flat, other.flat, m, self.lp)
        self.packer.run(self.flat)
        self.update_bn_affine()

    # ---- the same update in pieces (MoCo's key pipeline): parameters first, then the running statistics of one
    # group of BatchNorm layers at a time (each group's statistics and folded affine are contiguous: module order)
    @torch.no_grad()
    def ema_params_from(self, other, m):
        n = self.n_train
        ops.ema_update(self.flat[:n], other.flat[:n], m, self.lp[:n] if self.lp is not None else None)
        self.packer.run(self.flat)

    def bn_groups(self, groups):
        """groups: lists of sub-layers (in module order, together covering every BatchNorm of the arena) ->
        [(stat range in flat, affine range, index tensors)] for ema_stats_from."""
        out, pos = [], 0
        bns = [m for m in self.module.modules() if isinstance(m, _BatchNormBase) and m.affine]
        stat_start = {}
        off = self.n_train

        def aligned(n):
            return (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        for mod in [m for m in self.module.modules() if isinstance(m, _BatchNormBase)]:
            stat_start[id(mod)] = off
            off += 2 * aligned(mod.num_features)
        assert off == self.total
        done = 0
        for g in groups:
            mods = [m for sub in g for m in sub.modules() if isinstance(m, _BatchNormBase)]
            assert mods == bns[done:done + len(mods)], 'BatchNorm groups must follow the module order'
            s0 = stat_start[id(mods[0])]
            s1 = stat_start[id(mods[-1])] + 2 * aligned(mods[-1].num_features)
            a0 = mods[0]._rt.bn_slice[0]
            a1 = (mods[-1]._rt.bn_slice[1] + 7) // 8 * 8
            out.append(((s0, s1), (a0, a1), tuple(t[a0:a1].contiguous() for t in self._bn_idx)))
            done += len(mods)
        assert done == len(bns)
        return out

    @torch.no_grad()
    def ema_stats_from(self, other, m, group):
        (s0, s1), (a0, a1), idx = group
        ops.ema_update(self.flat[s0:s1], other.flat[s0:s1], m, None)
        if self.bn_affine is None:
            n = self._bn_idx[0].numel()
            self.bn_affine = (torch.empty(n, dtype=torch.float32, device=self.flat.device),
                              torch.empty(n, dtype=torch.float32, device=self.flat.device))
        ops.bn_fold(self.flat, idx, self._bn_eps, self.bn_affine[0][a0:a1], self.bn_affine[1][a0:a1])

    def _refresh_if_on_device(self):
        # Building a model on the host is allowed (config / registry / checkpoint tooling);
        # *running* it is not: refresh() and every layer raise on host tensors.
        if self.device.type == 'cuda':
            self.refresh()

    @torch.no_grad()
    def copy_from(self, other):
        self.flat.copy_(other.flat)
        self._refresh_if_on_device()
        self.update_bn_affine()

    @torch.no_grad()
    def update_bn_affine(self):
        if self._bn_idx is None:
            return
        n = self._bn_idx[0].numel()
        if self.bn_affine is None or self.bn_affine[0].numel() != n:
            self.bn_affine = (torch.empty(n, dtype=torch.float32, device=self.flat.device),
                              torch.empty(n, dtype=torch.float32, device=self.flat.device))
        if self.flat.is_cuda:
            ops.bn_fold(self.flat, self._bn_idx, self._bn_eps, *self.bn_affine)    # one launch, in place
        else:       # host-side model construction only (nothing runs there)
            g, b, m, v = (self.flat[i] for i in self._bn_idx)
            scale = g * torch.rsqrt(v + self._bn_eps)
            self.bn_affine[0].copy_(scale)
            self.bn_affine[1].copy_(b - m * scale)

    def clear_grad(self):
        if self.grads is not None:
            if self.grads.is_cuda:
                ops.fill_zero(self.grads)        # (a library launch: part of a recorded step plan)
            else:
                self.grads.zero_()

    def param_grad_ready(self, *params):
        """grad_ready for raw parameters (class / position embeddings, tokens, logit_scale ...) whose
        gradient is produced by one dedicated backward kernel: without the mark their bucket (and, since
        buckets launch in order, every later one) would only be reduced after the whole backward."""
        # through the same use counter as the layers' parameters: a Function whose forward ran twice in one step (two
        # views through one trunk) reports twice, and only the second report releases the bucket
        self.grad_ready([p._passl_index for p in params])

    def expect_grad(self, indices):
        """Called from the FORWARD of a layer (when autograd will run its backward) that will report ``grad_ready(indices)`` from its backward: a parameter
        used by several forward nodes of one step (SimSiam encodes its two views in two passes) receives one gradient
        contribution per use and is complete — ready for its all-reduce bucket — only after the last of them."""
        if self.reducer is not None:
            u = self._uses
            for i in indices:
                u[i] = u.get(i, 0) + 1

    def grad_ready(self, indices):
        """Called from the backward kernels' host code once the gradients of parameters
        `indices` (positions in param_slices) are enqueued on the compute stream."""
        if self.reducer is not None:
            u = self._uses
            for i in indices:
                left = u.get(i, 0) - 1
                if left > 0:
                    u[i] = left                # another forward use of this parameter has not run its backward yet
                    continue
                u.pop(i, None)
                self.reducer.mark_ready(i)
