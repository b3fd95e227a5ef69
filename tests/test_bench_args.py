"""bench.py's command line: a plain run measures the headline only; --full adds the legs beside it, each of which its own
--no-* flag still leaves out.  CPU only: the arguments are parsed, nothing runs."""
import pytest

import bench

EXTRAS = ('no_eager_leg', 'no_fp32_mode', 'no_kernel_profile', 'no_traffic', 'no_cpu_baseline')


def test_plain_run_skips_every_extra_leg():
    a = bench.parse_args(['--gpus', '1', '--steps', '5', '--warmup', '2'])
    assert not a.full and (a.steps, a.warmup) == (5, 2)
    assert all(getattr(a, k) for k in EXTRAS)


def test_full_run_keeps_every_leg_unless_left_out():
    a = bench.parse_args(['--full'])
    assert a.full and not any(getattr(a, k) for k in EXTRAS)
    a = bench.parse_args(['--full', '--no-traffic', '--no-cpu-baseline'])
    assert {k for k in EXTRAS if getattr(a, k)} == {'no_traffic', 'no_cpu_baseline'}


def test_dump_gemm_needs_the_kernel_profile_of_full(capsys):
    with pytest.raises(SystemExit):
        bench.parse_args(['--dump-gemm', 'shapes.json'])
    assert '--full' in capsys.readouterr().err
    assert bench.parse_args(['--full', '--dump-gemm', 'shapes.json']).dump_gemm == 'shapes.json'
