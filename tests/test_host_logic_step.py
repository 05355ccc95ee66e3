"""Host-side logic of FusedTrainer's step that needs no GPU: the one point at which the next batch's march is issued, the rule for
concentrated scenes shared by the trainer and RenderConfig."""
import pytest

POSITIONS = (0, 1, 2, 2.5, 2.75, 3, 4)          # in step order (ngp_hip/trainer.py: _PrefetchPoint)


@pytest.mark.parametrize("at", POSITIONS)
def test_prefetch_point_fires_once_at_its_position(at):
    from ngp_hip.trainer import _PrefetchPoint
    fired = []
    pf = _PrefetchPoint()
    pf.arm(at, lambda: fired.append(p))
    for p in POSITIONS:
        pf.reach(p)
    assert fired == [at]
    for p in POSITIONS:                           # a second walk (and any reach after firing) does nothing
        pf.reach(p)
    assert fired == [at]


def test_unarmed_prefetch_point_fires_nothing():
    from ngp_hip.trainer import _PrefetchPoint
    pf = _PrefetchPoint()
    for p in POSITIONS:
        pf.reach(p)
    assert pf.action is None
    fired = []
    pf.arm(3, lambda: fired.append(1))
    pf.reach(2.75)
    assert fired == [] and pf.action is not None  # armed, not yet reached
    pf.reach(3)
    pf.reach(3)
    pf.reach(4)
    assert fired == [1] and pf.action is None


def test_prefetch_point_is_disarmed_before_its_action_runs():
    """The action is taken off the point before it runs: an action that itself reaches a later position does not recurse."""
    from ngp_hip.trainer import _PrefetchPoint
    pf = _PrefetchPoint()
    fired = []

    def action():
        fired.append(1)
        pf.reach(4)
    pf.arm(1, action)
    pf.reach(1)
    assert fired == [1]


def test_concentrated_scene_rule_is_shared(monkeypatch):
    from ngp_hip import fused, trainer
    assert trainer.concentrated_scene is fused.concentrated_scene
    monkeypatch.delenv("NGP_EXPERIMENT", raising=False)
    assert not fused.concentrated_scene(0.0, 1)
    assert fused.concentrated_scene(1.0 / 256, 1) and fused.concentrated_scene(0.0, 6)
    for v, want in (("1", True), ("0", False)):
        monkeypatch.setenv("NGP_EXPERIMENT", "bwd_concentrated=" + v)
        assert fused.concentrated_scene(0.0, 1) is want and fused.concentrated_scene(1.0 / 256, 6) is want
