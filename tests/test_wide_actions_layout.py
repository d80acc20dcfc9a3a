"""Action widths 16..63 (wide head kernels): the flat parameter layout accepts them, counts the reference Agent's
parameters (cleanrl/ppo.py:71-123 sizes actor_mean / actor_logstd from the action space) and keeps every weight matrix on a
128-byte line; 0 and 64 are refused.  CPU only: catppo_mlp_layout_of touches no device."""
import pytest

from oracle import ppo_oracle as PO

ARCHS = [(512, 256, 128), (256, 256, 256)]


@pytest.mark.parametrize("hidden", ARCHS, ids=["ref", "3x256"])
@pytest.mark.parametrize("A", [16, 19, 37, 63])
def test_layout_accepts_wide_action_dims(A, hidden):
    from cat_envs import native
    D = 69
    lay = native.layout_of(native.shape_of(D, A, hidden))
    ag = PO.AgentOracle(D, A, hidden)
    assert lay.n_params == sum(p.numel() for p in ag.parameters())
    assert lay.off_logstd == 0 and lay.obs_pad == 80
    assert lay.out_dim[1][len(hidden)] == A and lay.out_dim[0][len(hidden)] == 1
    for net in range(2):
        for l in range(len(hidden) + 1):
            assert lay.off_w[net][l] * 4 % 128 == 0, (net, l)
            assert lay.off_b[net][l] % 4 == 0, (net, l)
            # segments in order, each inside the buffer, none overlapping the next
            assert lay.off_b[net][l] >= lay.off_w[net][l] + lay.out_dim[net][l] * lay.in_dim[l]
    assert lay.off_w[0][0] >= A
    assert lay.n_flat >= lay.off_b[1][len(hidden)] + A


@pytest.mark.parametrize("A", [0, 64, 100])
def test_layout_refuses_out_of_range_action_dims(A):
    from cat_envs import native
    with pytest.raises(ValueError, match="1 <= act_dim <= 63"):
        native.layout_of(native.shape_of(48, A, (256, 256, 256)))


def test_agent_builds_for_a_wide_action_space():
    """Agent(envs) of a plain env with 37 actions: sizes from the action space, the flat buffer ties every parameter"""
    from cat_envs.tasks.utils.cleanrl.ppo import Agent

    class _Space:
        def __init__(self, shape):
            self.shape = shape

    class _Env:
        num_envs = 8
        single_observation_space = {"policy": _Space((69,))}
        single_action_space = _Space((37,))

        @property
        def unwrapped(self):
            return self

    ag = Agent(_Env(), hidden=(512, 256, 128))
    assert ag.act_dim == 37 and ag.actor_logstd.shape == (1, 37)
    assert ag.actor_mean[-1].weight.shape == (37, 128)
    assert ag.n_params == sum(p.numel() for p in ag.parameters())
    assert ag.actor_logstd.data_ptr() == ag.flat.data_ptr()
