"""The A-operand prologue of the register-staged implicit-GEMM kernel (passl_hip_conv_igemm_apro): a BatchNorm's apply
pass done by the 1x1 convolution that consumes its output, forward (z = relu(y * scale + shift)) and backward
(dy = cA * g + cB * y + cC), with the transformed operand written back once for the weight gradient.

Every comparison is BIT FOR BIT (torch.equal on the raw bf16 / fp32 tensors) against the separate path built from the same
inputs — the streaming BatchNorm kernel followed by the plain convolution: both sides run the same device functions
(csrc/bn_chunk.h), and nothing downstream (convolution output, fused statistics, BatchNorm-backward slab, weight
gradient, a whole block's gradients and running statistics) may change by a bit.

Shapes: M = 3 * 7 * 7 = 147 rows = two 128-row tiles, the second one partial; one, two and four K-tiles; in the forward
form at least two column blocks (exactly one of them writes z, all compute from the same transform)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from passl_amd.hip import config as hip_config, lib as L, nn, ops, plan as P    # noqa: E402
from passl_amd.hip.packer import WeightPacker                                  # noqa: E402

DEV = 'cuda'
BF = torch.bfloat16
N, H, W = 3, 7, 7
M = N * H * W


def _bf(t):
    return t.to(DEV).to(BF)


def _packed(geom, descs, w):
    """w: [cout, cin, k, k] fp32 -> the packed bf16 operand of every launch in `descs`"""
    packer = WeightPacker()
    for d in descs:
        packer.add(0, geom.cout, geom.k, geom.k, geom.cin, d.pack)
    packer.build(DEV, BF).run(w.permute(0, 2, 3, 1).contiguous().to(DEV).view(-1))
    return packer


def _guarded(shape):
    """A NaN-filled bf16 tensor of `shape` with 128 more NaN rows behind it -> (tensor, guard rows)"""
    rows = shape[0] * shape[1] * shape[2]
    buf = torch.full((rows + 128, shape[3]), float('nan'), dtype=BF, device=DEV)
    return buf[:rows].view(shape), buf[rows:]


@pytest.fixture
def options():
    """set the flags igemm_a_bn / igemm_a_bnb (hip/config.py) for one test; the values they had come back afterwards"""
    before = {}

    def set_(**kw):
        for k, v in kw.items():
            before.setdefault(k, hip_config._state[k])
            hip_config.set_flag(k, v)
    yield set_
    for k, v in before.items():
        hip_config.set_flag(k, v)


# ======================================================================================== forward
@pytest.mark.parametrize('cin', [64, 128, 256])
def test_forward_prologue_is_bn_apply_then_conv(cin):
    geom = P.ConvGeom(cin, 4 * cin, 1, 1, 0)
    gen = torch.Generator().manual_seed(100 + cin)
    y = _bf(torch.randn(N, H, W, cin, generator=gen) * 1.5 + 0.3)
    gamma = (torch.rand(cin, generator=gen) + 0.5).to(DEV)
    beta = (torch.randn(cin, generator=gen) * 0.5).to(DEV)
    rm, rv = torch.zeros(cin, device=DEV), torch.ones(cin, device=DEV)
    w = torch.randn(geom.cout, cin, 1, 1, generator=gen) * 0.1
    fd = P.fwd_desc(geom, N, H, W)
    wp = _packed(geom, [fd], w).view(fd.pack, geom.cout)
    # separate path: the streaming apply pass, then the plain convolution with fused statistics
    z0, st, _ = ops.bn_train_fwd(y, gamma, beta, rm, rv, relu=True)
    clipped = float((z0 == 0).float().mean())
    assert 0.1 < clipped < 0.9, clipped                     # the ReLU clips a real share of the elements
    out0 = torch.empty(N, H, W, geom.cout, dtype=BF, device=DEV)
    slab0, tiles = ops.conv_stats_buffer(fd, DEV)
    ops.conv_igemm(fd, z0, wp, out0, stats=slab0)
    # one launch
    z1, guard = _guarded((N, H, W, cin))
    out1 = torch.full_like(out0, float('nan'))
    slab1 = torch.full_like(slab0, float('nan'))
    done = ops.conv_igemm(fd, y, wp, out1, stats=slab1, apro=dict(mode=1, scale=st[2], shift=st[3], out=z1))
    assert done is not None, 'the library refused the launch'
    assert L.load().passl_hip_last_igemm_kernel() == 0
    torch.cuda.synchronize()
    assert tiles == 2 and geom.cout // 128 >= 2
    assert torch.equal(z1, z0)
    assert torch.isnan(guard.float()).all()                 # rows m >= M are not stored
    assert torch.equal(out1, out0)
    n = tiles * geom.cout * 3
    assert torch.equal(slab1[:n], slab0[:n])


# ======================================================================================== backward
@pytest.mark.parametrize('with_bnb', [False, True])
@pytest.mark.parametrize('cout', [64, 256])
def test_backward_prologue_is_bn_bwd_apply_then_dgrad(cout, with_bnb):
    cin = 64
    geom = P.ConvGeom(cin, cout, 1, 1, 0)
    gen = torch.Generator().manual_seed(200 + cout + with_bnb)
    w = torch.randn(cout, cin, 1, 1, generator=gen) * 0.1
    dds, skipped = P.dgrad_plan(geom, N, H, W)
    assert len(dds) == 1 and not skipped
    d = dds[0]
    wp = _packed(geom, dds, w).view(d.pack, cin)
    # the BatchNorm behind the convolution: input y3 (the conv output), masked output gradient g, its reduced slab
    y3 = _bf(torch.randn(N, H, W, cout, generator=gen) * 1.3 + 0.2)
    g = _bf(torch.randn(N, H, W, cout, generator=gen) * (torch.rand(N, H, W, cout, generator=gen) > 0.4))
    gamma = (torch.rand(cout, generator=gen) + 0.5).to(DEV)
    beta = torch.zeros(cout, device=DEV)
    _z, st3, _ = ops.bn_train_fwd(y3, gamma, beta, torch.zeros(cout, device=DEV), torch.ones(cout, device=DEV),
                                  relu=False)
    nb = 4
    partial = torch.empty(ops.bn_partial_floats(nb, cout, False), dtype=torch.float32, device=DEV)
    L.check(L.load().passl_hip_bn_bwd_reduce(L.ptr(g), None, L.ptr(y3), L.ptr(st3[0]), L.ptr(st3[1]), None, None,
                                             L.ptr(partial), M, cout, nb, 0, L.dt(g), L.stream()), 'bn_bwd_reduce')
    # the BatchNorm in FRONT of the convolution (its backward statistics ride in the data gradient's epilogue), and
    # the residual-fork gradient added there
    x = _bf(torch.randn(N, H, W, cin, generator=gen))
    extra = _bf(torch.randn(N, H, W, cin, generator=gen))
    yp = _bf(torch.randn(N, H, W, cin, generator=gen) * 1.5 + 0.3)
    _zp, stp, _ = ops.bn_train_fwd(yp, (torch.rand(cin, generator=gen) + 0.5).to(DEV),
                                   torch.randn(cin, generator=gen).to(DEV), torch.zeros(cin, device=DEV),
                                   torch.ones(cin, device=DEV), relu=True)
    tiles = ops.conv_tiles(d)

    def bnb(slab):
        if not with_bnb:
            return None
        return dict(y=yp, mask=None, mean=stp[0], invstd=stp[1], scale=stp[2], shift=stp[3], relu=2, partial=slab,
                    tile_off=0)

    def slab_():
        return torch.full((ops.bn_partial_floats(tiles, cin, False),), float('nan'), dtype=torch.float32, device=DEV)
    # separate path: BatchNorm backward (finalize + apply pass), plain data gradient, weight gradient
    dg0, db0 = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
    dy0, _ = ops.bn_bwd(g, None, y3, gamma, st3[0], st3[1], dg0, db0, relu=0, fused=(partial, nb))
    dx0, s0 = torch.full((N, H, W, cin), float('nan'), dtype=BF, device=DEV), slab_()
    ops.conv_igemm(d, dy0, wp, dx0, residual=extra, bnb=bnb(s0))
    # deferred: finalize only, then ONE launch computes dy on its way in, writes it, and produces dx
    dg1, db1 = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
    dy1, _, coef = ops.bn_bwd(g, None, y3, gamma, st3[0], st3[1], dg1, db1, relu=0, fused=(partial, nb), defer=True)
    dy1g, guard = _guarded((N, H, W, cout))
    dx1, s1 = torch.full_like(dx0, float('nan')), slab_()
    done = ops.conv_igemm(d, g, wp, dx1, residual=extra, bnb=bnb(s1), apro=dict(mode=2, a2=y3, coef=coef, out=dy1g))
    assert done is not None, 'the library refused the launch'
    assert L.load().passl_hip_last_igemm_kernel() == 0
    torch.cuda.synchronize()
    assert torch.equal(dg1, dg0) and torch.equal(db1, db0)
    assert torch.equal(dy1g, dy0)
    assert torch.isnan(guard.float()).all()
    assert torch.equal(dx1, dx0)
    if with_bnb:
        assert torch.equal(s1[:tiles * cin * 2], s0[:tiles * cin * 2])
    # the weight gradient reads the written-back dy exactly as it reads the apply pass's
    wd = P.wgrad_desc(geom, N, H, W)
    dw0 = ops.zeros(cout, cin, dtype=torch.float32, device=DEV)
    dw1 = ops.zeros(cout, cin, dtype=torch.float32, device=DEV)
    ops.conv_wgrad(wd, x, dy0.view(-1, cout), dw0)
    ops.conv_wgrad(wd, x, dy1g.view(-1, cout), dw1)
    torch.cuda.synchronize()
    assert torch.equal(dw1, dw0) and float(dw0.abs().max()) > 0


# ======================================================================================== through nn.py
class _Spy:
    """counts the prologue launches ops.conv_igemm was asked for / the library took"""

    def __enter__(self):
        self.asked, self.taken = {1: 0, 2: 0}, {1: 0, 2: 0}
        self.reductions, self.off_main = [], 0         # of the backward launches taken: channels reduced; not on the main stream
        self.real = ops.conv_igemm
        main = torch.cuda.current_stream()

        def spy(*a, **kw):
            r = self.real(*a, **kw)
            if kw.get('apro') is not None:
                self.asked[kw['apro']['mode']] += 1
                self.taken[kw['apro']['mode']] += r is not None
                if r is not None and kw['apro']['mode'] == 2:
                    self.reductions.append(a[0].C)
                    self.off_main += torch.cuda.current_stream() != main
            return r
        ops.conv_igemm = spy
        return self

    def __exit__(self, *exc):
        ops.conv_igemm = self.real


def _init(module, seed):
    gen = torch.Generator().manual_seed(seed)
    arena = nn.EncoderArena(module, trainable=True)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 4:
                p.copy_((torch.randn(p.shape, generator=gen) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5).to(DEV))
            elif name.endswith('weight'):
                p.copy_((torch.rand(p.shape, generator=gen) + 0.5).to(DEV))
            else:
                p.copy_((torch.randn(p.shape, generator=gen) * 0.3).to(DEV))
    arena.refresh()
    return arena


def _step(module, arena, call, inputs, dout, input_grad=True):
    """One forward + backward from a fixed state -> every tensor the step leaves behind"""
    for m in module.modules():
        if isinstance(m, nn.BatchNorm2D):
            with torch.no_grad():
                m._mean.zero_()
                m._variance.fill_(1.0)
    arena.clear_grad()
    leaves = [t.detach().clone().requires_grad_(input_grad) for t in inputs]
    out = call(*leaves)
    out.backward(dout)
    torch.cuda.synchronize()
    got = {'out': out.detach().clone()}
    for i, t in enumerate(leaves):
        if input_grad:
            got['d-input %d' % i] = t.grad.clone()
    for name, p in module.named_parameters():
        got['d ' + name] = p.grad.clone()
    for name, b in module.named_buffers():
        got[name] = b.clone()
    return got


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_bottleneck_blocks_with_and_without_the_prologue(options):
    """Two stage-1 bottleneck blocks (the first with a downsample branch), forward + backward at N = 2, 8 x 8: every
    gradient and every BatchNorm running statistic is the same with both options on and off."""
    from passl_amd.modeling.backbones.resnet import BottleneckBlock
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(BF)
    ds = torch.nn.Sequential(nn.Conv2D(64, 256, 1, bias_attr=False), nn.BatchNorm2D(256))
    seq = torch.nn.Sequential(BottleneckBlock(64, 64, 1, ds), BottleneckBlock(256, 64))
    arena = _init(seq, 5)
    seq.train()
    gen = torch.Generator().manual_seed(6)
    x = _bf(torch.randn(2, 8, 8, 64, generator=gen))
    dout = _bf(torch.randn(2, 8, 8, 256, generator=gen))
    options(igemm_a_bn=7, igemm_a_bnb=7)
    with _Spy() as on:
        a = _step(seq, arena, seq, [x], dout)
    options(igemm_a_bn=0, igemm_a_bnb=0)
    with _Spy() as off:
        b = _step(seq, arena, seq, [x], dout)
    print('prologue launches taken: forward %d, backward %d' % (on.taken[1], on.taken[2]))
    assert on.taken[1] == 2                       # bn2 -> conv3 of both blocks
    # backward: conv1 (64 channels reduced), conv3 and the downsample convolution (256) of the first block; the last
    # BatchNorm of the second block gets its gradient from outside, unreduced, and applies it itself
    assert on.taken[2] == 3 and sorted(on.reductions) == [64, 256, 256]
    from passl_amd.hip import streams
    if streams.enabled(x) and hip_config.fork_downsample():
        assert on.off_main == 1                   # the downsample branch's backward runs on the side stream
    assert off.taken == {1: 0, 2: 0}
    _same(a, b)


class _Chain(nn.Layer):
    """conv_a -> BatchNorm + ReLU (+ residual) -> conv_b -> BatchNorm"""

    def __init__(self, cmid, stride):
        super().__init__()
        self.conv_a = nn.Conv2D(64, cmid, 1, bias_attr=False)
        self.bn_a = nn.BatchNorm2D(cmid)
        self.conv_b = nn.Conv2D(cmid, 128, 1, stride=stride, bias_attr=False)
        self.bn_b = nn.BatchNorm2D(128)
        self.defer = True

    def forward(self, x, res=None):
        y, st = self.conv_a(x, want_stats=True)
        z = self.bn_a(y, residual=res, relu=True, stats=st, consumer=self.conv_b if self.defer else None,
                      sole_reader=True)
        y2, st2 = self.conv_b(z, want_stats=True, producer=nn.bn_link(z), pending=nn.bn_pending(z))
        return self.bn_b(y2, relu=False, stats=st2)


@pytest.mark.parametrize('case', ['option_off', 'cin512', 'stride2', 'residual'])
def test_launches_outside_the_envelope_take_the_separate_path(case, options):
    """Option off, a reduction of eight K-tiles, a strided consumer, a BatchNorm with a residual input: no prologue
    launch, and the result of the chain is the one the classic call sequence gives."""
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(BF)
    cmid = 512 if case == 'cin512' else 64
    stride = 2 if case == 'stride2' else 1
    chain = _Chain(cmid, stride)
    arena = _init(chain, 11)
    chain.train()
    gen = torch.Generator().manual_seed(12)
    x = _bf(torch.randn(2, 8, 8, 64, generator=gen))
    ins = [x] + ([_bf(torch.randn(2, 8, 8, cmid, generator=gen))] if case == 'residual' else [])
    dout = _bf(torch.randn(2, 8 // stride, 8 // stride, 128, generator=gen))
    chain.defer = False                      # the classic sequence: the BatchNorm applies, the convolution reads z
    with _Spy() as ref:
        a = _step(chain, arena, chain, ins, dout)
    assert ref.asked[1] == 0
    chain.defer = True
    options(igemm_a_bn=0 if case == 'option_off' else 7)
    with _Spy() as got:
        b = _step(chain, arena, chain, ins, dout)
    assert got.taken[1] == 0
    _same(a, b)
    if case == 'option_off':
        # ... and with the option on this very chain does take the launch, with the same result
        options(igemm_a_bn=7)
        with _Spy() as on:
            c = _step(chain, arena, chain, ins, dout)
        assert on.taken[1] == 1
        _same(a, c)


@pytest.mark.parametrize('refuse', ['igemm_persist', 'no_input_grad'])
def test_fallbacks_give_the_separate_path(refuse, options):
    """The two ways a deferred apply pass comes back to the streaming kernel.  igemm_persist: the library refuses
    launches the call site holds eligible (the prologue has no persistent form): asked, not taken, forward and
    backward.  no_input_grad: the convolution in front of the BatchNorm has no data gradient to launch, so the
    deferred backward apply pass runs at the top of its backward.  Both bit for bit against both flags 0."""
    hip_config.set_device('gpu')
    hip_config.set_compute_dtype(BF)
    chain = _Chain(64, 1)
    arena = _init(chain, 21)
    chain.train()
    gen = torch.Generator().manual_seed(22)
    x = _bf(torch.randn(2, 8, 8, 64, generator=gen))
    dout = _bf(torch.randn(2, 8, 8, 128, generator=gen))
    grad = refuse != 'no_input_grad'
    if refuse == 'igemm_persist':
        L.set_option('igemm_persist', 1)
    try:
        options(igemm_a_bn=0, igemm_a_bnb=0)
        with _Spy() as ref:
            a = _step(chain, arena, chain, [x], dout, input_grad=grad)
        assert ref.asked == {1: 0, 2: 0}
        options(igemm_a_bn=7, igemm_a_bnb=7)
        with _Spy() as got:
            b = _step(chain, arena, chain, [x], dout, input_grad=grad)
    finally:
        L.set_option('igemm_persist', 0)
    if refuse == 'igemm_persist':
        assert got.asked == {1: 1, 2: 1} and got.taken == {1: 0, 2: 0}
    else:
        assert got.taken == {1: 1, 2: 0} and got.asked[2] == 0
    _same(a, b)
