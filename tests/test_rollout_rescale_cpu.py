"""``ga_policy_env_step_fused_f32`` under NormalizedEnv's action rescale, without a
GPU: with ``norm->act_low`` set the entry refuses missing bounds, a missing scratch
and a discrete env kind in ``ga_rollout_env_steps``' words, through ctypes with host
pointers -- each check precedes the first device call; and ``ga_rollout_env_steps``'
host loop against a kernel side that rescales inside the fused launch."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from garage_amd import _lib
from garage_amd.engine import FlatMLP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


def _args(kind, n=64, obs=3, out=1):
    """A call that passes every check but the rescale's (host pointers
    throughout: none of the calls below may reach a launch)."""
    net = FlatMLP(obs, out, (8, 8), CPU)
    buf = (C.c_float * 16)()
    addr = C.addressof(buf)
    head = _lib.HeadArgs(n=n, A=out, kind=0 if kind == 'pendulum' else 1,
                         obs=addr, ldo=4, obs_dim=obs, col=0, Tcap=8,
                         action=addr, lda=4, obs_buf=addr, act_buf=addr)
    rec = _lib.RecordArgs(
        n=n, col=0, Tcap=8, max_episode_length=5, reward=addr, step_type=addr,
        next_obs=addr, ldo=4, obs_dim=obs, ep_t=addr, rew_buf=addr,
        st_buf=addr, tail_buf=addr, lastobs_buf=addr, done=addr, step_eps=addr,
        step_samples=addr)
    if kind == 'pendulum':
        env = _lib.PendulumEnv(n=n, max_episode_length=5, state=addr, t=addr,
                               resets=addr)
        ref = _lib.env_ref(_lib.ENV_PENDULUM, env)
    else:
        env = _lib.CartPoleEnv(n=n, max_episode_length=5, state=addr, t=addr,
                               resets=addr)
        ref = _lib.env_ref(_lib.ENV_CARTPOLE, env)
    return dict(net=net, addr=addr, head=head, rec=rec, ref=ref, buf=buf)


def _call(a, norm, n_steps):
    _lib.call('ga_policy_env_step_fused_f32', C.byref(a['net']._desc), a['addr'],
              C.byref(a['head']), C.byref(a['ref']), C.byref(a['rec']),
              C.byref(norm), n_steps, None)


@pytest.mark.parametrize('n_steps', [1, 4])
def test_rescale_refusals_precede_the_launch(n_steps):
    name = 'ga_policy_env_step_fused_f32'
    a = _args('pendulum')
    p = a['addr']
    cases = {
        'null act_high': (a, _lib.NormArgs(act_low=p, scaled_action=p,
                                           expected_action_scale=1.0)),
        'null scaled_action': (a, _lib.NormArgs(act_low=p, act_high=p,
                                                expected_action_scale=1.0)),
    }
    b = _args('cartpole', obs=4)
    cases['discrete kind'] = (b, _lib.NormArgs(
        act_low=p, act_high=p, scaled_action=p, expected_action_scale=1.0))
    for what, (args, norm) in cases.items():
        with pytest.raises(_lib.GarageAmdError,
                           match='action rescale needs bounds, scratch and a '
                                 'continuous action space'):
            _call(args, norm, n_steps)
        assert name.encode() in _lib.load().ga_last_error(), what


def test_rescaled_rollout_loop_under_address_sanitizer():
    """``make asan-rescale-loop``: ga_rollout_env_steps' host loop compiled with
    ``-fsanitize=address,undefined`` against recording fakes of a kernel side that
    rescales inside the fused launch, as the library's does
    (tests/host/rollout_loop_harness.cpp, suite rescale-loop): one launch for a rescaled
    rollout, three per step with fusion off or teacher-forced noise, the
    refusals and their order."""
    out = subprocess.run(['make', '-C', ROOT, 'asan-rescale-loop'],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'all checks passed' in out.stdout
