"""GPU: the closed loop with the plant's inner-loop force feedback and an external push
(``ClosedLoop(feedback=True, push=True)``): 96 robots (the team solve path), 6 ticks, a wrench
written in place before tick 3.

Each tick's plant output is, bit for bit, a manual ``Plan.gain`` + ``Plan.srb_step(K=...)`` from
the tick's snapshot; two eager ticks and four replays of the captured graph are bit-identical to
six eager ticks; and the wrench written in place acts on a replay."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, TICKS, PUSH_AT = 96, 6, 3


def _loop(plan, **kw):
    from cmpc.closed_loop import ClosedLoop
    rng = np.random.default_rng(11)
    cl = ClosedLoop(B, plan=plan, seed=5, mu=rng.uniform(0.4, 0.9, B),
                    fz_min=rng.uniform(5.0, 12.0, B), **kw)
    cl.set_command(np.stack([rng.uniform(-0.5, 0.5, B), rng.uniform(-0.2, 0.2, B),
                             np.full(B, 0.27), rng.uniform(-1.0, 1.0, B)], 1))
    return cl


def _push(cl):
    import torch
    rng = np.random.default_rng(12)
    wrench = np.concatenate([rng.uniform(-60, 60, (B, 3)), rng.uniform(-8, 8, (B, 3))], 1)
    cl.wrench.copy_(torch.as_tensor(wrench, dtype=torch.float32))


def test_tick_is_gain_plus_srb_step(plan):
    import torch
    assert B <= plan.team_batch()
    cl = _loop(plan, feedback=True, push=True)
    assert cl.gain and torch.all(cl.wrench == 0)
    N = cl.N
    applied, moved = 0, 0
    for k in range(TICKS):
        if k == PUSH_AT:
            _push(cl)
        x, feet, contact, t = cl.x.clone(), cl.feet.clone(), cl.contact.clone(), cl.t.clone()
        cl.tick()
        assert torch.equal(cl.x_solve, x)
        K = plan.gain(cl.Ad, cl.Bd, cl.gd, cl.x_solve, cl.xref, cl.ct, w=cl.w, mu=cl.mu,
                      fz_min=cl.fz_min, want=("K",))["K"]
        assert torch.equal(K.view(torch.int64), cl.K0.view(torch.int64))
        status = torch.full((B,), 0xA5, dtype=torch.uint8, device=cl.dev)
        force = torch.empty((B, 12), dtype=torch.float32, device=cl.dev)
        plan.srb_step(t, cl.gait, cl.mass, cl.I_body, cl.w[:, 12 * N:], cl.hip, x, feet, contact,
                      cl.nsub, cl.dt / cl.nsub, K=K, x_solve=cl.x_solve, contact=cl.ct, mu=cl.mu,
                      fz_min=cl.fz_min, wrench=cl.wrench, fb_status=status, force_out=force)
        torch.cuda.synchronize()
        assert torch.equal(x, cl.x) and torch.equal(feet, cl.feet), k
        assert torch.equal(contact, cl.contact) and torch.equal(status, cl.fb_status), k
        assert int((cl.status != 1).sum()) == 0, k
        applied += int((status != 0).sum())
        # the law is not idle: the last substep's forces differ from the held U[:, 0]
        moved += int((force != cl.w[:, 12 * N:12 * N + 12]).any(1).sum())
    assert applied >= 0.9 * B * TICKS and moved >= 0.5 * B * TICKS, (applied, moved)
    assert bool(torch.isfinite(cl.x).all())


def test_graph_replay_matches_eager_and_takes_the_push(plan):
    import torch
    a, b, c = (_loop(plan, feedback=True, push=True) for _ in range(3))
    for k in range(TICKS):
        if k == 2:
            b.capture()
            c.capture()
        if k == PUSH_AT:
            _push(a)
            _push(b)                      # c is never pushed
        a.tick(); b.tick(); c.tick()
        assert b.graph is None if k < 2 else b.graph is not None
    torch.cuda.synchronize()
    for n in ("x", "feet", "contact", "w", "t", "K0", "fb_status"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert not torch.equal(b.x, c.x)
    # a 60 N push over three ticks of 1/48 s on a 15 kg body: of the order of 0.1 m/s
    dv = (b.x[:, 6:9] - c.x[:, 6:9]).abs().max().item()
    assert 0.01 < dv < 2.0, dv


def test_defaults_leave_the_tick_alone(plan):
    """feedback and push are off by default: no options reach the plant."""
    cl = _loop(plan)
    assert cl.plant == {} and not cl.gain and not hasattr(cl, "wrench")
    assert _loop(plan, gain=True).plant == {}
