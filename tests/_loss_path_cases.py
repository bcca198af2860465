"""The cases of ``test_loss_paths_fp64_gpu.py``: per update path, the smallest shapes
that reach its branches, with the objective's options walked across them so that each
path sees each option at least once.  ``check_tables`` states what the tables hold;
``test_loss_cases_cpu.py`` runs it without a GPU."""
from collections import OrderedDict, namedtuple

GATHER_POOL = 700

# dims: (inputs, hidden..., outputs); M: rows ('g': gathered with repeats out of
# GATHER_POOL); kind: 'gauss' / 'cat' / 'nll'; vpg: VPG's objective instead of PPO's;
# ent: None, 'reg_sp' (entropy regularised, through softplus) or 'max_stop' (maximum
# entropy with stop-gradient: the algorithms then add the entropy to the rewards and
# call the loss with ent_flags = 4 -- bit 0 off, no entropy term in the objective -- so
# through the paths these cases show that bit 2 alone is inert; stop-gradient with a
# live entropy term, flags 5 and 7, is what test_loss_entries_fp64_gpu.py pins);
# std: a key of _loss_cases.LOG_STD; dsm: double_softmax;
# learn_std: False registers the log-std as a buffer
P = namedtuple('P', 'dims M gather kind vpg ent std dsm learn_std')


def _p(dims, M, kind, vpg=False, ent=None, std='lo_inactive', dsm=1, learn_std=True):
    gather = isinstance(M, str)
    return P(tuple(dims), int(M[:-1]) if gather else M, gather, kind, vpg, ent, std, dsm,
             learn_std)


# narrow_step.hip: (O, 32, 32, A) and (O, 64, 64, A), O in {3, 32}, A in {1, 8},
# M in {1, 64, 65, 200 gathered}
NARROW = [
    _p((3, 32, 32, 1), 1, 'nll'),
    _p((32, 32, 32, 8), 64, 'gauss'),
    _p((3, 64, 64, 8), 65, 'cat', dsm=1),
    _p((32, 64, 64, 1), '200g', 'gauss', vpg=True, std='lo_active'),
    _p((3, 32, 32, 8), '200g', 'cat', dsm=0, ent='max_stop'),
    _p((32, 64, 64, 8), 65, 'gauss', ent='reg_sp', std='sp_free'),
    _p((3, 64, 64, 1), 64, 'nll'),
    _p((3, 32, 32, 8), 1, 'gauss', std='hi_active', learn_std=False),
    _p((32, 32, 32, 1), 65, 'gauss', std='at_lo'),
]
# fused_train.hip: last hidden layer 64 / 128 / 256, one to three hidden layers,
# M in {1, 127, 129, 513 gathered}, A in {1, 8}; 18 inputs at 256 x 256 is the pipelined
# k-loop
FUSED = [
    _p((12, 128, 8), 127, 'gauss'),
    _p((18, 256, 256, 8), '513g', 'gauss', ent='reg_sp'),
    _p((11, 128, 64, 128, 1), 129, 'nll'),
    _p((4, 64, 64, 8), 1, 'cat', dsm=1),
    _p((7, 96, 64, 1), 129, 'gauss', vpg=True, std='at_lo'),
    _p((5, 64, 128, 8), '513g', 'cat', dsm=0, ent='max_stop'),
    _p((17, 256, 256, 8), 127, 'gauss', std='hi_active'),
    _p((9, 128, 128, 8), 1, 'gauss', std='sp_hi_active'),
    _p((6, 64, 1), '513g', 'nll'),
    _p((10, 64, 128, 256, 8), 129, 'gauss', vpg=True, std='sp_free'),
    _p((9, 128, 128, 1), 127, 'gauss', std='lo_active', learn_std=False),
    _p((17, 256, 256, 8), 129, 'cat', dsm=1, vpg=True),
]
# small_step.hip: M in {1, 17, 64}, H in {32, 128, 256}
SMALL = [
    _p((4, 32, 32, 2), 64, 'cat', dsm=1),
    _p((17, 128, 128, 6), 17, 'gauss'),
    _p((8, 256, 256, 1), 1, 'nll'),
    _p((6, 128, 128, 3), 64, 'gauss', vpg=True, ent='reg_sp', std='sp_free'),
    _p((5, 32, 32, 8), 17, 'gauss', std='lo_active'),
    _p((5, 256, 256, 4), 64, 'gauss', std='hi_active', learn_std=False),
    _p((3, 32, 32, 1), 1, 'gauss', vpg=True, std='at_lo'),
    _p((7, 128, 128, 4), 1, 'cat', dsm=0, ent='max_stop'),
    _p((9, 256, 256, 1), 17, 'nll'),
    _p((9, 256, 256, 2), 17, 'gauss', vpg=True, std='sp_hi_active'),
]
# the head layer inside the loss kernel: hidden 64 and 512, A = 6
HEAD = [
    _p((9, 32, 64, 6), 129, 'gauss'),
    _p((9, 32, 512, 6), '513g', 'gauss', ent='reg_sp', std='sp_free'),
    _p((9, 512, 6), 1, 'gauss', vpg=True, std='hi_active'),
    _p((9, 32, 512, 1), 127, 'nll'),
    _p((9, 64, 1), '513g', 'nll'),
    _p((9, 32, 64, 6), 127, 'gauss', std='lo_active'),
    _p((9, 32, 512, 6), 129, 'gauss', vpg=True, ent='max_stop', std='at_lo'),
    _p((9, 64, 6), '513g', 'gauss', std='sp_hi_active', learn_std=False),
    _p((9, 512, 512, 6), 1, 'gauss', ent='max_stop', learn_std=False),
]
# the per-layer kernels: every case above, and A = 9, which the fused paths refuse
PER_LAYER = list(OrderedDict.fromkeys(NARROW + FUSED + SMALL + HEAD + [
    _p((6, 64, 64, 9), 65, 'gauss'),
    _p((6, 64, 64, 9), '200g', 'cat', dsm=1, ent='max_stop'),
]))


def case_id(p):
    bits = ['x'.join(str(d) for d in p.dims), 'M%d%s' % (p.M, 'g' if p.gather else ''),
            p.kind, 'vpg' if p.vpg else 'ppo']
    if p.kind == 'gauss':
        bits.append(p.std)
    if p.kind == 'cat':
        bits.append('dsm%d' % p.dsm)
    if p.ent:
        bits.append(p.ent)
    if not p.learn_std:
        bits.append('fixed_std')
    return '-'.join(bits)


def check_tables():
    def opts(cases):
        return {(c.kind, c.vpg) for c in cases}, {c.ent for c in cases}, {
            c.std for c in cases if c.kind == 'gauss'}, {
                c.dsm for c in cases if c.kind == 'cat'}, {c.learn_std for c in cases}
    for cases in (NARROW, FUSED, SMALL, HEAD, PER_LAYER):
        kinds, ents, stds, dsms, learn = opts(cases)
        assert kinds >= {('gauss', False), ('gauss', True), ('nll', False)}
        assert ents == {None, 'reg_sp', 'max_stop'}
        # (the head-in-loss kernels have no categorical form)
        assert dsms == (set() if cases is HEAD else {0, 1})
        # inactive and active lower clamp, active upper clamp, softplus std
        assert stds >= {'lo_inactive', 'lo_active', 'hi_active'}
        assert stds & {'sp_free', 'sp_hi_active'} and learn == {True, False}
    assert all(c.dims[1] == c.dims[2] for c in NARROW)
    assert {c.dims[1] for c in NARROW} == {32, 64}
    assert {c.dims[0] for c in NARROW} == {3, 32} and {c.dims[-1] for c in NARROW} == {1, 8}
    assert {c.M for c in NARROW} == {1, 64, 65, 200}
    assert {c.dims[-2] for c in FUSED} == {64, 128, 256}
    assert {len(c.dims) - 2 for c in FUSED} == {1, 2, 3}
    assert {c.M for c in FUSED} == {1, 127, 129, 513}
    assert {c.dims[-1] for c in FUSED} == {1, 8} and (18, 256, 256, 8) in {
        c.dims for c in FUSED}
    assert {(c.M, c.dims[1]) for c in SMALL} == {(M, H) for M in (1, 17, 64)
                                                 for H in (32, 128, 256)}
    assert {c.M for c in SMALL if c.kind == 'nll'} >= {1, 17}
    assert {c.dims[-2] for c in HEAD} == {64, 512}
    assert {c.dims[-1] for c in HEAD if c.kind == 'gauss'} == {6}
    assert any(c.dims[-1] == 9 for c in PER_LAYER)
