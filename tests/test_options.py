"""The library's tuning options (passl_amd/csrc/options.h): every name and default, the PASSL_<NAME> environment
variables, and the one switch that Python and the library share (wgrad_halo).  Each case runs in a fresh process: the
library reads the environment once, on the first access to any option.  No GPU involved."""
import json
import os
import re
import subprocess
import sys

import pytest

from passl_amd.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'passl_hip.h')
OPTIONS_H = os.path.join(ROOT, 'passl_amd', 'csrc', 'options.h')

# the spec: every option and its default
DEFAULTS = {
    'igemm_ring': 1, 'igemm_ring_min_nk': 8, 'igemm_ring_min_tiles': 1, 'igemm_ring_bm': 128, 'igemm_ring_bk': 64,
    'igemm_ring_stages32': 4,
    'igemm_8p': 1, 'igemm_8p_min_nk': 8, 'igemm_8p_direct': 1, 'igemm_8p_dense': 1, 'igemm_8p_tk': 145,
    'igemm_8p_te': 1000, 'igemm_8p_te_direct': 900, 'igemm_8p_ring_tk': 112, 'igemm_8p_ring_te': 420,
    'igemm_8p_margin': 100,
    'conv3x3_wave': 1, 'conv3x3_wave_rows': 4, 'conv3x3_wave_modes': 7, 'conv3x3_wave_dbg': 0,
    'igemm_persist': 0, 'igemm_persist_grid': 0, 'igemm_nk1': 24, 'igemm_lean': 1, 'igemm_dbg': 0,
    'stem_kernel': 1,
    'wgrad_dma': 1, 'wgrad_tile': 0, 'wgrad_pipe': 2, 'wgrad_halo': 2, 'wgrad_halo_stages': 2, 'wgrad_dbg': 0,
    'bn_stream_unroll': 4,
    'stem_pool_form': 1, 'stem_pool_wgs': 1024,
    'attn_f32mfma': 0, 'attn_waves': 0,
}

# an accepted value other than the default, per option
OTHER = {
    'igemm_ring': 0, 'igemm_ring_min_nk': 4, 'igemm_ring_min_tiles': 2, 'igemm_ring_bm': 256, 'igemm_ring_bk': 32,
    'igemm_ring_stages32': 3,
    'igemm_8p': 2, 'igemm_8p_min_nk': 4, 'igemm_8p_direct': 0, 'igemm_8p_dense': 2, 'igemm_8p_tk': 150,
    'igemm_8p_te': 1100, 'igemm_8p_te_direct': 950, 'igemm_8p_ring_tk': 120, 'igemm_8p_ring_te': 400,
    'igemm_8p_margin': 90,
    'conv3x3_wave': 0, 'conv3x3_wave_rows': 8, 'conv3x3_wave_modes': 5, 'conv3x3_wave_dbg': 1,
    'igemm_persist': 1, 'igemm_persist_grid': 16, 'igemm_nk1': 12, 'igemm_lean': 0, 'igemm_dbg': 2,
    'stem_kernel': 0,
    'wgrad_dma': 0, 'wgrad_tile': 3, 'wgrad_pipe': 1, 'wgrad_halo': 1, 'wgrad_halo_stages': 3, 'wgrad_dbg': 1,
    'bn_stream_unroll': 8,
    'stem_pool_form': 0, 'stem_pool_wgs': 512,
    'attn_f32mfma': 1, 'attn_waves': 4,
}

# prints {name: value} of the options named in argv, read through passl_hip_get_option (ctypes only: no torch)
_READ = r'''
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = {}
for name in sys.argv[2:]:
    v = ctypes.c_int(-12345)
    assert lib.passl_hip_get_option(name.encode(), ctypes.byref(v)) == 0, name
    out[name] = v.value
print(json.dumps(out))
'''


@pytest.fixture(scope='module')
def libpath():
    if not os.path.exists(L.LIB_PATH):
        from passl_amd.csrc.build import build
        build()
    return L.LIB_PATH


def clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('PASSL_')}
    env.update(extra)
    return env


def read_options(libpath, names, env):
    r = subprocess.run([sys.executable, '-c', _READ, libpath] + list(names), env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), r.stderr


def test_the_spec_lists_every_option_of_the_table():
    table = dict((n, int(d)) for n, d in re.findall(r'^\s*X\((\w+),\s*(-?\d+),', open(OPTIONS_H).read(), flags=re.M))
    assert len(table) == 37
    assert table == DEFAULTS
    assert sorted(OTHER) == sorted(DEFAULTS) and all(OTHER[n] != DEFAULTS[n] for n in DEFAULTS)


def test_defaults_and_their_documentation(libpath):
    values, err = read_options(libpath, DEFAULTS, clean_env())
    assert values == DEFAULTS
    assert 'libpassl_hip' not in err
    doc = open(HEADER).read()
    doc = doc[doc.index('Tuning and diagnostic options'):doc.index('int passl_hip_set_option(')]
    for name in DEFAULTS:
        assert re.search(r'\*\s+%s\s' % name, doc), 'option %s is not listed in include/passl_hip.h' % name


def test_every_option_reads_its_environment_variable(libpath):
    env = clean_env(**{'PASSL_' + n.upper(): str(v) for n, v in OTHER.items()})
    values, err = read_options(libpath, OTHER, env)
    assert values == OTHER
    assert 'libpassl_hip' not in err


def test_a_bad_environment_value_keeps_the_default(libpath):
    values, err = read_options(libpath, ['bn_stream_unroll', 'igemm_ring', 'igemm_8p'],
                               clean_env(PASSL_BN_STREAM_UNROLL='3', PASSL_IGEMM_RING='on', PASSL_IGEMM_8P='2'))
    assert values == {'bn_stream_unroll': 4, 'igemm_ring': 1, 'igemm_8p': 2}
    assert 'bn_stream_unroll' in err and 'PASSL_BN_STREAM_UNROLL=3' in err
    assert 'PASSL_IGEMM_RING=on' in err and 'PASSL_IGEMM_8P' not in err


def test_get_option_refuses_unknown_names_and_null(libpath):
    lib = L.load()
    import ctypes
    v = ctypes.c_int()
    assert lib.passl_hip_get_option(b'no_such_option', ctypes.byref(v)) == L.EINVAL
    assert lib.passl_hip_get_option(b'wgrad_halo', None) == L.EINVAL
    assert lib.passl_hip_get_option(None, ctypes.byref(v)) == L.EINVAL


def test_python_and_library_agree_on_wgrad_halo(libpath):
    """config.set_flag before load() wins even when PASSL_OPTIONS names another wgrad_halo_* option (advisor finding:
    a substring test once skipped the push)."""
    code = ('from passl_amd.hip import config, lib as L\n'
            'config.set_flag("wgrad_halo", 1)\n'
            'L.load()\n'
            'print(L.get_option("wgrad_halo"), config.wgrad_halo(), L.get_option("wgrad_halo_stages"))\n')
    r = subprocess.run([sys.executable, '-c', code], env=clean_env(PASSL_OPTIONS='wgrad_halo_stages=3'), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ['1', '1', '3']
