"""The SATCV_* variables of the Python package (satellite_computervision_amd/switches.py): every default, every reading, every read time,
one reader of the environment, and table = DESIGN.md appendix = consumers.

Everything expected here is written by hand from the expressions the six consumer files held before the table existed
(`os.environ.get(V, d) != '0'`, `== '1'`, `int(...)`, ...), never computed by the code under test."""
import ast
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'satellite_computervision_amd')
ERR = ValueError            # "this text raises ValueError", in the tables below

# the readings of '0', '1', '2', a word and the empty string under the parse idioms the consumers used
ON = {'0': False, '1': True, '2': True, 'x': True, '': True}            # os.environ.get(V, '1') != '0'   (PREFETCH, LSTM_GRAPH: not == '0')
ONLY = {'0': False, '1': True, '2': False, 'x': False, '': False}      # os.environ.get(V, d) == '1'
INT = {'0': 0, '1': 1, '2': 2, '-3': -3, ' 7 ': 7, 'x': ERR, '': ERR}           # int(os.environ.get(V, d))
TEXT = {'0': '0', '1': '1', '2': '2', 'x': 'x', '': ''}                         # os.environ.get(V, d)

# key: (variable, default as the appendix prints it, read time, value when unset, {text: value})
PINNED = {
    'bn_bias_noise': ('SATCV_BN_BIAS_NOISE', '0', 'import', False, ONLY),
    'ctbf': ('SATCV_CTBF', '1', 'import', True, ON),
    'ctbf_couts': ('SATCV_CTBF_COUTS', '`32,64`', 'import', (32, 64),
                   {'0': (0,), '1': (1,), '2': (2,), '32,,64,': (32, 64), '': (), ',': (), '16': (16,), 'x': ERR, '32,x': ERR}),
    'fuse_residual': ('SATCV_FUSE_RESIDUAL', '1', 'import', True, ONLY),
    'fuse_dgrad_bn_bwd': ('SATCV_FUSE_DGRAD_BN_BWD', '1', 'import', 1, {'0': 0, '1': 1, '2': 2, 'x': 1, '': 1, '02': 1, '3': 1}),
    'wgrad_last_full': ('SATCV_WGRAD_LAST_FULL', '1', 'plan', True, ON),
    'deeplab_splitk': ('SATCV_DEEPLAB_SPLITK', '1', 'model', True, ONLY),
    'prefetch': ('SATCV_PREFETCH', '1', 'call', True, ON),
    'fuse_head_bn_bwd': ('SATCV_FUSE_HEAD_BN_BWD', '1', 'model', True, ON),
    'wgrad_stream': ('SATCV_WGRAD_STREAM', '1', 'model', True, ON),
    'fuse_pool_bn_sums': ('SATCV_FUSE_POOL_BN_SUMS', '1', 'model', True, ON),
    'fuse_head_grad': ('SATCV_FUSE_HEAD_GRAD', '1', 'model', True, ON),
    'fuse_pool_bwd': ('SATCV_FUSE_POOL_BWD', '1', 'model', True, ON),
    'fuse_thin_bwd': ('SATCV_FUSE_THIN_BWD', '1', 'model', True, ON),
    'sync_bn': ('SATCV_SYNC_BN', '0', 'model', False, ONLY),
    'folded_infer': ('SATCV_FOLDED_INFER', '1', 'call', True, ON),
    'infer_graph': ('SATCV_INFER_GRAPH', '1', 'call', 1, INT),
    'infer_graph_min': ('SATCV_INFER_GRAPH_MIN', '64', 'call', 64, INT),
    'fp8_scaled': ('SATCV_FP8_SCALED', '1', 'import', True, ON),
    'fuse_pool': ('SATCV_FUSE_POOL', '1', 'import', True, ON),
    'fp8_hybrid': ('SATCV_FP8_HYBRID', '1', 'import', True, ON),
    'fp8_thin': ('SATCV_FP8_THIN', '1', 'import', True, ON),
    'siamese_pair': ('SATCV_SIAMESE_PAIR', '1', 'import', True, ON),
    'force_collectives': ('SATCV_FORCE_COLLECTIVES', '0', 'import', False, ONLY),
    'cabi_comm': ('SATCV_CABI_COMM', '0', 'import', False, ONLY),
    'grad_payload': ('SATCV_GRAD_PAYLOAD', '`fp32`', 'call', 'fp32', dict(TEXT, bf16='bf16')),
    'overlap_allreduce': ('SATCV_OVERLAP_ALLREDUCE', '1', 'call', True, ON),
    'lstm_recurrent_activation': ('SATCV_LSTM_RECURRENT_ACTIVATION', '`hard_sigmoid`', 'import', 'hard_sigmoid', dict(TEXT, sigmoid='sigmoid')),
    'lstm_graph': ('SATCV_LSTM_GRAPH', '1', 'call', True, ON),
    'lib': ('SATCV_LIB', 'unset', 'import', None, dict(TEXT, **{'/a/b.so': '/a/b.so'})),
}
KEYS = (       # the 30, in the order of the appendix
    'bn_bias_noise', 'ctbf', 'ctbf_couts', 'fuse_residual', 'fuse_dgrad_bn_bwd', 'wgrad_last_full', 'deeplab_splitk', 'prefetch', 'fuse_head_bn_bwd',
    'wgrad_stream', 'fuse_pool_bn_sums', 'fuse_head_grad', 'fuse_pool_bwd', 'fuse_thin_bwd', 'sync_bn', 'folded_infer', 'infer_graph',
    'infer_graph_min', 'fp8_scaled', 'fuse_pool', 'fp8_hybrid', 'fp8_thin', 'siamese_pair', 'force_collectives', 'cabi_comm', 'grad_payload',
    'overlap_allreduce', 'lstm_recurrent_activation', 'lstm_graph', 'lib')
CLASSES = {'production', 'opt-in feature', 'compatibility aid', 'test aid', 'profiling aid'}

# the import-time module constants at their defaults, and in a process that has every `import` row at another value (IMPORT_ENV)
_LIB_DEFAULT = os.path.join(PKG, 'libsatcv.so')
CONSTANTS = {
    'engine': dict(BIAS_NOISE=False, CTBF=True, CTBF_COUTS=[32, 64], FUSE_RESIDUAL=True, FUSE_DGRAD_ALL=False),
    'fp8_infer': dict(USE_SCALED_MFMA=True, FUSE_POOL=True, HYBRID=True, THIN_FP8=True, SIAMESE_PAIR=True),
    'parallel': dict(FORCE=False, CABI_COMM=False),
    'lstm_tools': dict(RECURRENT_ACTIVATION='hard_sigmoid'),
    '_lib': dict(LIB_PATH=_LIB_DEFAULT)}
IMPORT_ENV = {
    'SATCV_BN_BIAS_NOISE': '1', 'SATCV_CTBF': '0', 'SATCV_CTBF_COUTS': '16,', 'SATCV_FUSE_RESIDUAL': '2',
    'SATCV_FUSE_DGRAD_BN_BWD': '2', 'SATCV_FP8_SCALED': '0', 'SATCV_FUSE_POOL': '0', 'SATCV_FP8_HYBRID': '0', 'SATCV_FP8_THIN': '0',
    'SATCV_SIAMESE_PAIR': '0', 'SATCV_FORCE_COLLECTIVES': '1', 'SATCV_CABI_COMM': '1', 'SATCV_LSTM_RECURRENT_ACTIVATION': 'sigmoid'}      # + SATCV_LIB
CONSTANTS_CHANGED = {
    'engine': dict(BIAS_NOISE=True, CTBF=False, CTBF_COUTS=[16], FUSE_RESIDUAL=False, FUSE_DGRAD_ALL=True),
    'fp8_infer': dict(USE_SCALED_MFMA=False, FUSE_POOL=False, HYBRID=False, THIN_FP8=False, SIAMESE_PAIR=False),
    'parallel': dict(FORCE=True, CABI_COMM=True),
    'lstm_tools': dict(RECURRENT_ACTIVATION='sigmoid')}         # + _lib.LIB_PATH


def _clear(monkeypatch):
    for v in [v for v in os.environ if v.startswith('SATCV_')]:
        monkeypatch.delenv(v)


def _constants_in_child(env):
    """the import-time constants of a fresh process whose only SATCV_* variables are `env`"""
    code = ('import sys, json, importlib; sys.path.insert(0, %r)\n'
            'want = json.loads(%r); got = {}\n'
            'for m, names in want.items():\n'
            '    mod = importlib.import_module("satellite_computervision_amd." + m)\n'
            '    got[m] = {n: getattr(mod, n) for n in names}\n'
            'print(json.dumps(got))' % (ROOT, json.dumps({m: sorted(c) for m, c in CONSTANTS.items()})))
    clean = {k: v for k, v in os.environ.items() if not k.startswith('SATCV_')}
    r = subprocess.run([sys.executable, '-c', code], env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_table_holds_its_keys():
    from satellite_computervision_amd import switches
    rows = switches.rows()
    assert tuple(r.key for r in rows) == KEYS and len(KEYS) == 30 and set(KEYS) == set(PINNED)
    assert len({r.env for r in rows}) == 30
    for r in rows:
        env, _, when, _, _ = PINNED[r.key]
        assert (r.env, r.when) == (env, when), r.key
        assert r.cls in CLASSES and r.meaning and callable(r.reader), r.key
    with pytest.raises(KeyError):
        switches.read('no_such_switch')
    src = open(os.path.join(PKG, 'switches.py')).read()
    imported = {a.name for n in ast.walk(ast.parse(src)) if isinstance(n, ast.Import) for a in n.names} | \
               {n.module for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ImportFrom)}
    assert imported == {'os', 'collections'}, imported          # _lib.py imports it: no torch, no _lib


def test_defaults_are_pinned(monkeypatch):
    from satellite_computervision_amd import switches
    _clear(monkeypatch)
    got = {k: switches.read(k) for k in KEYS}
    assert got == {k: p[3] for k, p in PINNED.items()}
    for k in KEYS:
        assert type(got[k]) is type(PINNED[k][3]), k


def test_import_time_constants_at_their_defaults():
    assert _constants_in_child({}) == CONSTANTS


@pytest.mark.parametrize('key', KEYS)
def test_parsing_is_pinned(key, monkeypatch):
    from satellite_computervision_amd import switches
    _clear(monkeypatch)
    env, _, _, _, readings = PINNED[key]
    assert {'0', '1', '2'} <= set(readings) and len(readings) >= 4
    for text, want in readings.items():
        monkeypatch.setenv(env, text)
        if want is ERR:
            with pytest.raises(ValueError):
                switches.read(key)
        else:
            got = switches.read(key)
            assert got == want and type(got) is type(want), (key, text, got)


def test_the_quirks_the_consumers_depend_on(monkeypatch):
    from satellite_computervision_amd import switches
    _clear(monkeypatch)

    def at(var, text, key):
        monkeypatch.setenv(var, text)
        return switches.read(key)
    assert at('SATCV_FUSE_RESIDUAL', '2', 'fuse_residual') is False and at('SATCV_CTBF', '2', 'ctbf') is True
    assert at('SATCV_CTBF_COUTS', '32,,64,', 'ctbf_couts') == (32, 64) and at('SATCV_CTBF_COUTS', '', 'ctbf_couts') == ()
    for text, want in (('0', (False, False)), ('1', (True, False)), ('2', (True, True))):
        v = at('SATCV_FUSE_DGRAD_BN_BWD', text, 'fuse_dgrad_bn_bwd')
        assert (v != 0, v == 2) == want            # (Model.fuse_dgrad_bn_bwd, engine.FUSE_DGRAD_ALL)
    for var, key in (('SATCV_PREFETCH', 'prefetch'), ('SATCV_LSTM_GRAPH', 'lstm_graph')):
        assert [at(var, t, key) for t in ('0', '1', '2', 'off', '')] == [False, True, True, True, True]


MODEL_FLAGS = {'fuse_head_bn_bwd': 'SATCV_FUSE_HEAD_BN_BWD', 'fuse_dgrad_bn_bwd': 'SATCV_FUSE_DGRAD_BN_BWD', 'wgrad_side_stream': 'SATCV_WGRAD_STREAM',
               'fuse_pool_bn_sums': 'SATCV_FUSE_POOL_BN_SUMS', 'fuse_head_grad': 'SATCV_FUSE_HEAD_GRAD', 'fuse_pool_bwd': 'SATCV_FUSE_POOL_BWD',
               'fuse_thin_bwd': 'SATCV_FUSE_THIN_BWD'}


def test_later_rows_are_read_when_they_are_used(monkeypatch):
    """plan / model / call rows see a variable set after the import; the import-time constants do not"""
    from satellite_computervision_amd import switches, engine, fp8_infer, parallel, lstm_tools, _lib, model_tools as mt
    mods = {'engine': engine, 'fp8_infer': fp8_infer, 'parallel': parallel, 'lstm_tools': lstm_tools, '_lib': _lib}
    before = {m: {n: getattr(mods[m], n) for n in names} for m, names in CONSTANTS.items()}
    _clear(monkeypatch)
    # model rows, through their consumer: Model.__init__ and the DeepLab builder
    m = mt.get_unet_model(2, 4)
    assert [getattr(m, a) for a in MODEL_FLAGS] == [True] * 7 and m.sync_bn is False
    assert mt.get_deeplabv3_model(2, 4)._infer_splitk is True
    for var in MODEL_FLAGS.values():
        monkeypatch.setenv(var, '0')
    monkeypatch.setenv('SATCV_SYNC_BN', '1')
    monkeypatch.setenv('SATCV_DEEPLAB_SPLITK', '0')
    m = mt.get_unet_model(2, 4)
    assert [getattr(m, a) for a in MODEL_FLAGS] == [False] * 7 and m.sync_bn is True
    assert mt.get_deeplabv3_model(2, 4)._infer_splitk is False
    monkeypatch.setenv('SATCV_FUSE_DGRAD_BN_BWD', '2')
    assert mt.get_unet_model(2, 4).fuse_dgrad_bn_bwd is True
    # a call row through its consumer: the wire format of a GradSync built now
    assert parallel.GradSync(10).payload == 'fp32'
    monkeypatch.setenv('SATCV_GRAD_PAYLOAD', 'bf16')
    assert parallel.GradSync(10).payload == 'bf16' and parallel.GradSync(10, payload='fp32').payload == 'fp32'
    # every plan / model / call row at another value than its default
    late = {'wgrad_last_full': ('0', False), 'deeplab_splitk': ('0', False), 'prefetch': ('0', False), 'fuse_head_bn_bwd': ('0', False),
            'wgrad_stream': ('0', False), 'fuse_pool_bn_sums': ('0', False), 'fuse_head_grad': ('0', False), 'fuse_pool_bwd': ('0', False),
            'fuse_thin_bwd': ('0', False), 'sync_bn': ('1', True), 'folded_infer': ('0', False), 'infer_graph': ('2', 2), 'infer_graph_min': ('8', 8),
            'grad_payload': ('bf16', 'bf16'), 'overlap_allreduce': ('0', False), 'lstm_graph': ('0', False)}
    assert set(late) == {k for k, p in PINNED.items() if p[2] != 'import'}
    for k, (text, want) in late.items():
        assert want != PINNED[k][3]
        monkeypatch.setenv(PINNED[k][0], text)
        assert switches.read(k) == want, k
    # the import rows: read() sees the late value, the module constants keep what the import read
    for var, text in dict(IMPORT_ENV, SATCV_LIB='/nowhere/libsatcv_variant.so').items():
        monkeypatch.setenv(var, text)
    assert switches.read('ctbf') is False and switches.read('lib') == '/nowhere/libsatcv_variant.so'
    assert {m: {n: getattr(mods[m], n) for n in names} for m, names in CONSTANTS.items()} == before


def test_import_rows_are_read_at_import(tmp_path):
    """a fresh process with every import row at another value than its default: every module constant follows"""
    assert set(IMPORT_ENV) | {'SATCV_LIB'} == {p[0] for p in PINNED.values() if p[2] == 'import'}
    variant = str(tmp_path / 'libsatcv_variant.so')
    shutil.copy(_LIB_DEFAULT, variant)
    got = _constants_in_child(dict(IMPORT_ENV, SATCV_LIB=variant))
    assert got == dict(CONSTANTS_CHANGED, _lib=dict(LIB_PATH=variant))
    for m in CONSTANTS_CHANGED:
        for n, v in CONSTANTS_CHANGED[m].items():
            assert v != CONSTANTS[m][n], (m, n)
    assert _constants_in_child({'SATCV_LIB': ''})['_lib'] == dict(LIB_PATH=_LIB_DEFAULT)          # `... or <the library beside the package>`
    assert _constants_in_child({'SATCV_FUSE_DGRAD_BN_BWD': '0'})['engine']['FUSE_DGRAD_ALL'] is False


# ------------------------------------------------------------------ one reader
ALLOWED = {'switches.py': None, 'parallel.py': {'WORLD_SIZE', 'LOCAL_RANK'}, 'build.py': {'HIPCC'}}         # None: any variable
SITES = {'engine.py': 6, 'model_tools.py': 13, 'fp8_infer.py': 5, 'parallel.py': 4, 'lstm_tools.py': 2, '_lib.py': 1}


def _package_sources():
    for d, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith('.py'):
                p = os.path.join(d, f)
                yield os.path.relpath(p, PKG), ast.parse(open(p).read(), p)


def test_one_reader_of_the_environment_in_the_package():
    seen = set()
    for rel, tree in _package_sources():
        parent = {c: n for n in ast.walk(tree) for c in ast.iter_child_nodes(n)}
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module == 'os':
                assert not {a.name for a in n.names} & {'environ', 'getenv', 'environb', 'putenv'}, rel
            if isinstance(n, ast.Name):
                assert n.id not in ('environ', 'getenv'), (rel, n.lineno)
            if not (isinstance(n, ast.Attribute) and n.attr in ('environ', 'environb', 'getenv', 'putenv', 'unsetenv')):
                continue
            assert rel in ALLOWED, f'{rel}:{n.lineno} reads the environment: it belongs in switches.py'
            seen.add(rel)
            if ALLOWED[rel] is None:
                continue
            # os.environ.get('NAME', ...) / os.environ['NAME'] / os.getenv('NAME', ...) with an allowed literal name, nothing else
            up = parent[n]
            if n.attr == 'environ' and isinstance(up, ast.Attribute) and up.attr == 'get' and isinstance(parent[up], ast.Call):
                arg = parent[up].args[0]
            elif n.attr == 'environ' and isinstance(up, ast.Subscript) and isinstance(up.ctx, ast.Load):
                arg = up.slice
            elif n.attr == 'getenv' and isinstance(up, ast.Call):
                arg = up.args[0]
            else:
                raise AssertionError(f'{rel}:{n.lineno}: not a plain read of one variable')
            assert isinstance(arg, ast.Constant) and arg.value in ALLOWED[rel], (rel, n.lineno, ast.dump(arg))
    assert seen == set(ALLOWED)


def test_every_row_has_its_consumers():
    """every read goes through switches.read('<literal key>'): 31 sites, each key once and SATCV_FUSE_DGRAD_BN_BWD in engine.py and model_tools.py"""
    sites = []
    for rel, tree in _package_sources():
        for n in ast.walk(tree):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'read' and getattr(n.func.value, 'id', None) == 'switches':
                assert len(n.args) == 1 and isinstance(n.args[0], ast.Constant), (rel, n.lineno)
                sites.append((rel, n.args[0].value))
    assert {f: sum(1 for r, _ in sites if r == f) for f in {r for r, _ in sites}} == SITES
    keys = sorted(k for _, k in sites)
    assert keys == sorted(KEYS + ('fuse_dgrad_bn_bwd',))
    assert {r for r, k in sites if k == 'fuse_dgrad_bn_bwd'} == {'engine.py', 'model_tools.py'}


# ------------------------------------------------------------------ table = appendix
def test_table_and_appendix_agree():
    from satellite_computervision_amd import switches
    doc = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert 'untouched by the table' not in doc
    doc = doc[doc.index('### Python side'):]
    doc = doc[:doc.index('Outside both tables')]
    found = re.findall(r'^\| `(SATCV_\w+)` \| `(\w+)` \| (\S+) \| (\w+) \| ([^|]+) \| (.*) \|$', doc, re.M)
    assert len(found) == len([l for l in doc.splitlines() if l.startswith('| `')]) == 30
    by_key = {f[1]: f for f in found}
    assert set(by_key) == set(KEYS) == {r.key for r in switches.rows()}
    for r in switches.rows():
        var, _, default, when, cls, meaning = by_key[r.key]
        assert (var, when, cls) == (r.env, r.when, r.cls), r.key
        assert default == PINNED[r.key][1] == ('unset' if r.default is None else r.default if re.fullmatch(r'-?\d+', r.default) else f'`{r.default}`'), r.key
        assert meaning.endswith(': ' + r.meaning), r.key
    assert '`SATCV_RCCL_LIB`' in open(os.path.join(ROOT, 'DESIGN.md')).read() and 'SATCV_RCCL_LIB' not in {r.env for r in switches.rows()}
    assert 'switches.rows()' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
