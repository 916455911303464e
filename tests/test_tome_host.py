"""Token merging without a GPU: parse_r against values recorded from the reference, the host arithmetic of a patched
pass, the float64 restatement of tome_util against itself (two formulations) and the preconditions every GPU case
relies on — each seeded matching case is decided 16 times over in float64 alone."""
import math

import numpy as np
import pytest
import torch

import tome_util as U
from passl_amd.models.utils import tome

# passl/models/utils/tome.py parse_r, run as it stands (plain Python, no framework involved)
PARSE_R = [
    ((12, 16), [16] * 12),
    ((12, 0), [0] * 12),
    ((12, 8), [8] * 12),
    ((12, (16, -1)), [32, 29, 26, 23, 20, 17, 14, 11, 8, 5, 2, 0]),
    ((12, (16, 1)), [0, 2, 5, 8, 11, 14, 17, 20, 23, 26, 29, 32]),
    ((12, (16, 0)), [16] * 12),
    ((12, (13, -0.5)), [19, 17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7]),
    ((24, (8, -1)), [16, 15, 14, 13, 13, 12, 11, 11, 10, 9, 9, 8, 7, 6, 6, 5, 4, 4, 3, 2, 2, 1, 0, 0]),
    ((3, [4, 3]), [4, 3, 0]),
    ((3, [4, 3, 0]), [4, 3, 0]),
    ((2, [1, 2, 3]), [1, 2, 3]),
]


@pytest.mark.parametrize('args, want', PARSE_R)
def test_parse_r_is_the_reference_arithmetic(args, want):
    assert tome.parse_r(*args) == want


def test_parse_r_does_not_alias_or_modify_its_list():
    r = [4, 3]
    out = tome.parse_r(3, r)
    assert r == [4, 3] and out is not r


@pytest.mark.parametrize('T, r, depth', [(197, 16, 12), (197, (16, -1), 12), (37, [4, 3, 0], 3), (50, 40, 4), (3, 5, 3)])
def test_token_schedule(T, r, depth):
    rs = tome.parse_r(depth, r)
    r_i, t_in, t_final = tome.token_schedule(T, rs)
    assert (r_i, t_in, t_final) == U.schedule(T, rs)
    assert t_in[0] == T and t_final == T - sum(r_i)
    for ri, ti, want in zip(r_i, t_in, rs):
        assert 0 <= ri <= (ti - 1) // 2 and ri == min(want, (ti - 1) // 2)
        assert ti - ri >= 2 or ti < 3                   # the class token and one more always remain
    # the class row of image b after the pass
    assert [b * t_final for b in range(3)] == [0, t_final, 2 * t_final]


def test_vit_b16_r16_ends_with_11_tokens():
    assert tome.token_schedule(197, tome.parse_r(12, 16))[2] == 11
    assert tome.token_schedule(197, tome.parse_r(12, (16, -1)))[2] == 197 - sum(tome.parse_r(12, (16, -1)))


def test_unsupported_token_kinds_raise():
    q = torch.zeros(2 * 5, 3 * 32)
    with pytest.raises(NotImplementedError):
        tome.bipartite_soft_matching(q, 1, 2, 5, 1, 32, class_token=False)
    with pytest.raises(NotImplementedError):
        tome.bipartite_soft_matching(q, 1, 2, 5, 1, 32, distill_token=True)
    assert tome.bipartite_soft_matching(q, 0, 2, 5, 1, 32) is None
    assert tome.bipartite_soft_matching(q, 3, 2, 2, 1, 32) is None       # two tokens: the clamp is 0


# ------------------------------------------------------------------ the restatement against a second formulation
def _loop_match(qkv, r):
    """bipartite_soft_matching step by step in Python floats, one image at a time."""
    B, T = qkv.shape[:2]
    out = []
    for b in range(B):
        m = qkv[b, :, 1].double().mean(dim=1)
        m = m / m.norm(dim=-1, keepdim=True)
        A, Bt = list(range(0, T, 2)), list(range(1, T, 2))
        nm, ni = [], []
        for i in A:
            sc = [-math.inf if i == 0 else float(m[i] @ m[j]) for j in Bt]
            best = max(sc)
            nm.append(best)
            ni.append(sc.index(best))
        order = sorted(range(len(A)), key=lambda i: (-nm[i], i))
        src = set(order[:r])
        unm = [i for i in range(len(A)) if i not in src]
        dest = [0] * T
        for row, i in enumerate(unm):
            dest[A[i]] = row
        for j in range(len(Bt)):
            dest[Bt[j]] = len(unm) + j
        for i in src:
            dest[A[i]] = len(unm) + ni[i]
        out.append(dest)
    return np.array(out)


@pytest.mark.parametrize('T, r', [(3, 1), (17, 4), (18, 8), (37, 18)])
def test_float64_matching_two_ways(T, r):
    qkv = U.make_qkv('random', 2, T, 2, 32, 100 + T)
    res = U.match(qkv, r)
    assert np.array_equal(res['dest'], _loop_match(qkv, r))
    assert res['dest'][:, 0].tolist() == [0, 0]                              # the class token stays row 0
    for b in range(2):
        assert sorted(set(res['dest'][b].tolist())) == list(range(T - r))   # every output row has a source
        unm = [t for t in range(0, T, 2) if not res['merged'][b, t // 2]]
        assert [res['dest'][b, t] for t in unm] == list(range(len(unm)))    # unmerged A tokens first, ascending


def test_float64_merge_is_merge_wavg():
    """merge_wavg as the reference writes it: x * size scattered and summed, sizes likewise, then the quotient."""
    B, T, r, C = 2, 17, 5, 8
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(B, T, C, generator=gen).double()
    size = U.previous_sizes(B, T, 9)
    dest = U.random_dest(B, T, r, 4)
    got = U.merge(x, size, dest, T - r)
    for b in range(B):
        for row in range(T - r):
            src = [t for t in range(T) if dest[b, t] == row]
            s = sum(float(size[b, t]) for t in src)
            y = sum(x[b, t] * float(size[b, t]) for t in src) / s
            assert torch.allclose(got['y'][b, row], y, rtol=1e-14, atol=0)
            assert float(got['size_out'][b, row]) == s and float(got['n'][b, row]) == len(src)
    assert float(got['size_out'].sum()) == float(size.sum())
    # the gradient restatement is the vector-Jacobian product of that merge
    xg = x.clone().requires_grad_(True)
    d = torch.as_tensor(dest)
    num = torch.zeros(B, T - r, C, dtype=torch.float64).scatter_add(1, d.unsqueeze(-1).expand(B, T, C),
                                                                    xg * size.double().unsqueeze(-1))
    y = num / got['size_out'].unsqueeze(-1)
    dy = torch.randn(B, T - r, C, generator=gen).double()
    y.backward(dy)
    assert torch.allclose(U.merge_bwd(dy, size, got['size_out'], dest)['dx'], xg.grad, rtol=1e-13, atol=0)


def test_keybias_reference_with_zero_bias_is_plain_attention():
    import attention_util as A
    qkv, dout = A.make_inputs('plain', 2, 17, 3, 32, 5)
    ref = A.reference(qkv, dout, 32 ** -0.5, False)
    got = U.keybias_reference(qkv, torch.zeros(2, 17), 32 ** -0.5)
    assert torch.allclose(got['out'], ref['out'], rtol=1e-13, atol=1e-15)
    assert torch.allclose(got['lse'], ref['lse'], rtol=1e-13, atol=0)
    # a bias of log 2 on one key is that key counted twice
    bias = torch.zeros(2, 17)
    bias[:, 5] = math.log(2.0)
    twice = torch.cat([qkv, qkv[:, 5:6]], dim=1)
    want = A.reference(twice, torch.cat([dout, dout[:, :1]], dim=1), 32 ** -0.5, False)['out'][:, :17]
    assert torch.allclose(U.keybias_reference(qkv, bias, 32 ** -0.5)['out'], want, rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------ preconditions of the GPU cases
@pytest.mark.parametrize('case', U.MATCH_CASES, ids=[U.match_case_id(c) for c in U.MATCH_CASES])
def test_every_seeded_matching_case_is_decided_in_float64(case):
    T, r, B, H, DH = case
    qkv, res, mg, seed = U.match_case(case)
    assert torch.equal(qkv, U.bf16_round(qkv))                   # the same values in fp32 and in bf16
    assert mg == U.margin(DH, H, res['kappa_max']) and mg < 1e-3
    assert U.smallest_gap(res) >= U.GAP_FACTOR * 2 * mg
    assert int(res['merged'].sum()) == B * r and not res['merged'][:, 0].any()
    assert res['dest'].min() == 0 and res['dest'].max() == T - r - 1


def test_the_special_matching_cases():
    qkv, res, mg, _ = U.norm_case()
    T, r, B, H, DH = U.NORM_CASE
    assert U.smallest_gap(res) >= U.GAP_FACTOR * 2 * mg
    k = qkv[:, :, 1].double()
    assert float(k[:, 4].norm(dim=-1).min()) ** 2 > 3.5e38 and float(k[:, 8].norm(dim=-1).max()) ** 2 < 1.4e-45
    tie = U.tie_case()
    m, _ = U.metric(tie)
    s = np.einsum('bid,bjd->bij', m[:, 0::2], m[:, 1::2])
    s[:, 0] = -np.inf
    top = np.sort(s.max(axis=-1), axis=-1)
    assert np.all(np.abs(top[:, -2:] - 1.0) < 1e-12) and np.all(top[:, -3] < 0.9)   # two rows tie at 1, the rest are far


@pytest.mark.parametrize('case', U.MERGE_CASES, ids=[U.merge_case_id(c) for c in U.MERGE_CASES])
def test_every_merge_case_is_a_valid_matching_result(case):
    T, r, B, C, sizes = case
    d = U.merge_case(case)
    assert d['dest'].shape == (B, T) and d['dest'].min() == 0 and d['dest'].max() == T - r - 1
    assert float(d['fwd']['n'].min()) >= 1 and float(d['fwd']['n'].sum()) == B * T
    if d['size'] is not None:
        assert torch.equal(d['size'], d['size'].round()) and float(d['size'].min()) >= 1
    so = d['fwd']['size_out']
    assert torch.equal(so, so.round()) and float(so.max()) < 2 ** 24          # exact in fp32


# ------------------------------------------------------------------ against the run of the reference's own tome.py
def test_parse_r_against_the_recorded_reference_values():
    import tome_model_util as MU
    fx = MU.load(MU.LAYERS)
    for tag, n, arg in (('int16', 12, 16), ('dec16', 12, (16, -1)), ('inc16', 12, (16, 1)), ('half13', 12, (13, -0.5)),
                        ('list', 3, [4, 3])):
        assert tome.parse_r(n, arg) == fx['parse_r/' + tag].tolist(), tag


def test_restatement_against_the_reference_layer_fixtures():
    """tests/golden/tome_layers.npz: the reference's bipartite_soft_matching and merge_wavg on recorded inputs.  The
    float64 restatement gives the same indices, scores, merged rows and sizes."""
    import tome_model_util as MU
    fx = MU.load(MU.LAYERS)
    for n, (B, T, H, DH, C, r, prev) in enumerate(MU.LAYER_CASES):
        pre = 'case%d/' % n
        qkv, x = torch.from_numpy(fx[pre + 'qkv']), torch.from_numpy(fx[pre + 'x'])
        size = torch.from_numpy(fx[pre + 'size'])[..., 0] if prev else None
        res = U.match(qkv, r)
        want = MU.dest_from_indices(T, fx[pre + 'unm_idx'], fx[pre + 'src_idx'], fx[pre + 'dst_idx'])
        assert np.array_equal(res['dest'], want), n
        assert np.array_equal(res['node_idx'][:, 1:], fx[pre + 'node_idx'][:, 1:]), n
        assert np.allclose(res['node_max'][:, 1:], fx[pre + 'node_max'][:, 1:], rtol=0, atol=1e-13), n
        got = U.merge(x, size, res['dest'], T - r)
        assert torch.allclose(got['y'], torch.from_numpy(fx[pre + 'y']), rtol=1e-12, atol=1e-14), n
        assert torch.equal(got['size_out'], torch.from_numpy(fx[pre + 'new_size'])[..., 0]), n
        if prev:
            assert float(size.max()) > 1 and float(size.sum()) == B * (T + 5)


def test_model_fixture_is_consistent_with_the_host_arithmetic():
    import tome_model_util as MU
    fx = MU.load(MU.FIXTURE)
    r_i, t_in, t_final = tome.token_schedule(MU.TOKENS, tome.parse_r(MU.MODEL['depth'], list(MU.R)))
    assert r_i == fx['r'].tolist() and t_in == fx['t_in'].tolist() and t_final == int(fx['t_final'])
    assert float(fx['gap']) >= 4 * float(fx['change']) > 0
    for tag in ('s0', 'prop'):
        for i, (r, T) in enumerate((r, T) for r, T in zip(r_i, t_in) if r > 0):
            pre = '%s/layer%d/' % (tag, i)
            dest = MU.dest_from_indices(T, fx[pre + 'unm_idx'], fx[pre + 'src_idx'], fx[pre + 'dst_idx'])
            assert dest.shape == (MU.BATCH, T) and sorted(set(dest[0].tolist())) == list(range(T - r))
            assert np.all(dest[:, 0] == 0)
