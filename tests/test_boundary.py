"""CPU checks of the drop-in boundary: the C-ABI library exports every symbol of
include/genrl_hip.h, the product modules reproduce the reference's weight contract, and the
product path fails loudly (no CPU fallback) when asked to compute without the MI355X."""
import ctypes, os
import pytest
import torch

import param_shapes
from oracle import genrl_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_header_symbols():
    from genrl_amd import _lib, build
    build.build(verbose=False)
    decl = _lib.parse_header()
    assert len(decl) >= 30
    L = ctypes.CDLL(_lib.SO)
    for name in decl:
        assert hasattr(L, name), name
    _lib.lib()   # argtypes bind


@pytest.mark.parametrize('tiny', [True, False])
def test_weight_contract(tiny):
    from genrl_amd import config
    over = config.tiny_overrides() if tiny else {}
    cfg = config.default_cfg(2, 16, device='cpu', **over)
    ag = config.make_agent(cfg)
    mine = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    ocfg = O.make_cfg(stoch=4, discrete=4, deter=32, hidden=32, units=32, cnn_depth=4) if tiny else O.make_cfg()
    ref = param_shapes.agent_param_shapes(ocfg)
    assert mine == ref
    assert not any(p.requires_grad for p in ag.parameters())
    if not tiny:
        n = lambda pre: sum(v.numel() for k, v in ag.state_dict().items() if k.startswith(pre))
        assert n('wm.') == 43328162 and n('_imag_behavior.actor.') == 5275668 and n('_imag_behavior.critic.') == 5516543


def test_no_cpu_fallback():
    from genrl_amd import ops, _lib
    with pytest.raises(_lib.GenrlHipError):
        ops.linear(torch.randn(4, 8), torch.randn(3, 8), None)


def test_no_cpu_fallback_refuses_before_any_launch(monkeypatch):
    """as on a machine WITH a GPU (the current stream resolves): host tensors are refused before the library is reached, so no kernel
    is ever launched on host addresses"""
    from genrl_amd import ops, _lib

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'library reached ({name}) with host tensors')
    monkeypatch.setattr(ops, '_stream', lambda: 0)
    monkeypatch.setattr(ops, 'lib', lambda: NoLib())
    for f in (lambda: ops.linear(torch.randn(4, 8), torch.randn(3, 8), None),
              lambda: ops.linear(torch.randn(4, 8), torch.randn(3, 8), torch.randn(3)),
              lambda: ops.copy2d(torch.randn(4, 8), 8, torch.empty(4, 8), 8, 4, 8)):
        with pytest.raises(_lib.GenrlHipError):
            f()


def test_agent_is_picklable():
    import io
    from genrl_amd import config
    cfg = config.default_cfg(2, 16, device='cpu', **config.tiny_overrides())
    ag = config.make_agent(cfg)
    buf = io.BytesIO(); torch.save(ag, buf); buf.seek(0)
    ag2 = torch.load(buf, weights_only=False)
    assert set(ag2.state_dict()) == set(ag.state_dict())


def test_dreamer_agent_weight_contract():
    from genrl_amd import config
    cfg = config.dreamer_cfg(2, 18, device='cpu', **config.dreamer_tiny_overrides())
    ag = config.make_dreamer_agent(cfg)
    ocfg = O.make_cfg(stoch=4, discrete=4, act_dim=6, deter=32, hidden=32, units=32, cnn_depth=4,
                      single_obs_posterior=False, decoder_inputs='feat')
    assert {k: tuple(v.shape) for k, v in ag.state_dict().items()} == param_shapes.agent_param_shapes(ocfg, dreamer=True)


# ---- the argument structs of the C launch loops: their ctypes classes come from the header (genrl_amd/_lib.py), filled through ops.fill

STRUCTS = ('genrl_planes_ref', 'genrl_rollout', 'genrl_rollout_bwd', 'genrl_rollout_f32', 'genrl_observe', 'genrl_split_desc',
           'genrl_reduce_desc')


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every field's offset of every struct the parser finds against a host program that includes the header (the compiler is
    the reference, not the parser's own output: this is what catches a mis-read declaration)"""
    import subprocess
    from genrl_amd import _lib
    S = _lib.structs()
    assert set(STRUCTS) <= set(S)
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "genrl_hip.h"', 'int main() {']
    for name, cls in S.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    (tmp_path / 'layout.cpp').write_text('\n'.join(lines + ['  return 0;', '}', '']))
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.cpp'),
                           '-o', str(tmp_path / 'layout')])
    want = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).splitlines())
    mine = {}
    for name, cls in S.items():
        mine[name] = str(ctypes.sizeof(cls))
        mine.update({f'{name}.{f}': str(getattr(cls, f).offset) for f, _ in cls._fields_})
    assert len(want) == len(mine) > 280 and mine == want


def test_fill_refuses_unknown_fields_host_and_strided_tensors(monkeypatch):
    from genrl_amd import ops, _lib

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f'library reached ({name}) with host tensors')
    monkeypatch.setattr(ops, '_stream', lambda: 0)
    monkeypatch.setattr(ops, 'lib', lambda: NoLib())
    a = _lib.struct('genrl_rollout')()
    ops.fill(a, H=3, unimix=0.5, stoch=None, deter=4096)          # scalars, NULL, an address that was already offset
    ops.fill(a, at=2, pU=7, pb=None)
    assert (a.H, a.unimix, a.stoch, a.deter, a.pU[2], a.pb[2]) == (3, 0.5, None, 4096, 7, None)
    for kw in (dict(stohc=None), dict(H=1, orr_=None)):            # a misspelt name sets nothing on a ctypes instance: refused instead
        with pytest.raises(AttributeError):
            ops.fill(a, **kw)
    with pytest.raises(AttributeError):
        ops.fill(a, at=0, pww=None)
    for cls in _lib.structs().values():                            # ... and on plain assignment too, array elements included
        for inst in (cls(), (cls * 2)()[1]):
            with pytest.raises(AttributeError):
                inst.no_such_field = 1
    with pytest.raises(AttributeError):
        a.pw[1].ldd = 64
    with pytest.raises(_lib.GenrlHipError):                        # host tensor: refused before the library is reached
        ops.fill(a, stoch=torch.randn(4, 8))
    with pytest.raises(_lib.GenrlHipError):
        ops.fill(a, at=1, pb=torch.randn(8))

    class OnGpu:                                                   # (what _p looks at: no device is needed to be refused for strides)
        is_cuda = True

        def is_contiguous(self):
            return False

        def data_ptr(self):
            raise AssertionError('address of a non-contiguous tensor taken')
    with pytest.raises(AssertionError, match='non-contiguous'):
        ops._p(OnGpu())
    with pytest.raises(AssertionError, match='non-contiguous'):
        ops.fill(a, stoch=OnGpu())


def test_struct_pointer_argtypes_refuse_other_structs():
    from genrl_amd import _lib
    decl = _lib.parse_header()
    entries = {'genrl_imagine_seq_fwd': 'genrl_rollout', 'genrl_imagine_seq_bwd': 'genrl_rollout_bwd',
               'genrl_imagine_seq_f32_fwd': 'genrl_rollout_f32', 'genrl_imagine_seq_f32_bwd': 'genrl_rollout_f32',
               'genrl_observe_seq_fwd': 'genrl_observe', 'genrl_observe_seq_bwd': 'genrl_observe',
               'genrl_split_h2_batch': 'genrl_split_desc', 'genrl_reduce_params_batch': 'genrl_reduce_desc'}
    for fn, sname in entries.items():
        at, cls = decl[fn][1][0][0], _lib.struct(sname)
        assert at is ctypes.POINTER(cls), fn
        for ok in (cls(), (cls * 3)(), ctypes.byref(cls()), None):
            at.from_param(ok)
        other = _lib.struct('genrl_observe' if sname != 'genrl_observe' else 'genrl_rollout')
        for bad in (other(), (other * 3)(), ctypes.byref(other()), ctypes.c_void_p(4096), 4096, ctypes.addressof(cls())):
            with pytest.raises((TypeError, ctypes.ArgumentError)):
                at.from_param(bad)
    _lib.lib()                       # and the bound library carries exactly these argtypes
    assert _lib.lib().genrl_imagine_seq_fwd.argtypes[0] is ctypes.POINTER(_lib.struct('genrl_rollout'))


@pytest.mark.parametrize('body', ['int a : 3;', 'double x;', 'struct { int a; } in;', 'union { int a; float b; } u;', 'float* a, b;',
                                  'float** pp;', 'unsigned int n;', 'int (*fn)(int);', 'genrl_later v;', 'int a[N];', 'int a\n#if 1\n;'])
def test_struct_parser_refuses_what_is_outside_its_grammar(tmp_path, body):
    from genrl_amd import _lib
    h = tmp_path / 'h.h'
    h.write_text('typedef struct { int ok; const float* p; float e[8]; } genrl_first;\n'
                 'typedef struct { genrl_first f; %s } genrl_t;\nint genrl_f(const genrl_t* t, void* stream);\n' % body)
    with pytest.raises(ValueError):
        _lib.parse_header(path=str(h))
    h.write_text('typedef struct { int ok; const float* p; float e[8]; } genrl_first;\n'
                 'typedef struct { genrl_first f; /* %s */ long n, m; } genrl_t;\nint genrl_f(const genrl_t* t, void* stream);\n' % body)
    assert _lib.parse_header(path=str(h))['genrl_f'][1][0][0] is ctypes.POINTER(_lib.structs(str(h))['genrl_t'])
