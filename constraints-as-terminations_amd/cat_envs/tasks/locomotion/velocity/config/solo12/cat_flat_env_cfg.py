"""Solo12 flat-terrain CaT task: constraint and curriculum configuration.

The ``ConstraintsCfg`` / ``CurriculumCfg`` below carry the reference's values
(solo12/cat_flat_env_cfg.py:259-355 and :383-451: 13 terms / 78 columns, 8 annealed terms).
Scene, physics, events and observation *terms* of the reference need Isaac Sim /
PhysX (NVIDIA only) and are out of scope; ``SyntheticCfg`` configures the device-resident
synthetic stream that stands in for the simulator.  Rewards: the stream simulator's are
a pre-generated stream; on the servo surrogate ``RewardsCfg`` (the reference's two terms and values)
or any other block of ``mdp.rewards`` terms is evaluated inside the simulator's launch
(``Solo12ServoRewardsFlatEnvCfg``, DESIGN section 9 "Rewards").  Observations: likewise, ``ObservationsCfg``
(the reference's six terms, order, scales and noise ranges) is evaluated inside the servo simulator's launch
(``Solo12ServoObsFlatEnvCfg``, DESIGN section 9 "Observations").  Events: ``EventCfg`` (the reference's four terms and
values) likewise (``Solo12ServoEventsFlatEnvCfg``, DESIGN section 9 "Events"); ``Solo12ServoFullFlatEnvCfg`` puts the three
blocks together.  Commands: ``CommandsCfg`` (the reference's ``UniformVelocityCommandWithDeadzoneCfg`` and values) likewise
(``Solo12ServoCommandsFlatEnvCfg``, DESIGN section 9 "Commands"); ``Solo12ServoReferenceFlatEnvCfg`` is all four blocks.
Terminations: ``TerminationsCfg`` (the reference's three terms and values) likewise (``Solo12ServoTerminationsFlatEnvCfg``,
DESIGN section 9 "Terminations"); ``Solo12ServoReferenceTerminationsFlatEnvCfg`` is all five blocks.
Actions: ``ActionsCfg`` (the reference's ``JointPositionActionCfg`` and values) likewise (``Solo12ServoActionsFlatEnvCfg``,
DESIGN section 9 "Actions"); ``Solo12ServoReferenceActionsFlatEnvCfg`` is all six blocks.
Actuators: ``scene.robot`` (the reference's ``SOLO12_MINIMAL_CFG``: one ideal PD group, its gains, armature and limits)
likewise (``Solo12ServoActuatorsFlatEnvCfg``, DESIGN section 9 "Actuators"); ``Solo12ServoReferenceActuatorsFlatEnvCfg`` is
all six blocks and the robot, ``Solo12ServoDelayedActuatorsFlatEnvCfg`` the same gains behind an actuator delay.
Randomisation: ``RandomizationEventCfg`` (per-env gains, joint friction and base mass; this project's ranges) likewise
(``Solo12ServoRandomizedFlatEnvCfg``, DESIGN section 9 "Randomisation"); ``Solo12ServoReferenceRandomizedFlatEnvCfg`` adds
the three terms to the reference's ``EventCfg`` on all six blocks and the robot.
"""
import math

from cat_envs.assets.odri import SOLO12_MINIMAL_CFG
from cat_envs.shim import AdditiveUniformNoiseCfg as Unoise
from cat_envs.shim import CurriculumTermCfg as CurrTerm
from cat_envs.shim import EventTermCfg as EventTerm
from cat_envs.shim import ObservationGroupCfg as ObsGroup
from cat_envs.shim import ObservationTermCfg as ObsTerm
from cat_envs.shim import RewardTermCfg as RewTerm
from cat_envs.shim import DelayedPDActuatorCfg, SceneEntityCfg, configclass
from cat_envs.shim import TerminationTermCfg as DoneTerm
from cat_envs.tasks.utils.cat import constraints, curriculums
from cat_envs.tasks.utils.cat.manager_constraint_cfg import ConstraintTermCfg as ConstraintTerm
from cat_envs.tasks.utils.mdp import actions, commands, events, observations, rewards, terminations

ALL_JOINTS = [".*_HAA", ".*_HFE", ".*_KFE"]


@configclass
class ConstraintsCfg:
    # Safety soft constraints
    joint_torque = ConstraintTerm(func=constraints.joint_torque, max_p=0.25,
                                  params={"limit": 3.0, "asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    joint_velocity = ConstraintTerm(func=constraints.joint_velocity, max_p=0.25,
                                    params={"limit": 16.0, "asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    joint_acceleration = ConstraintTerm(func=constraints.joint_acceleration, max_p=0.25,
                                        params={"limit": 800.0,
                                                "asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    action_rate = ConstraintTerm(func=constraints.action_rate, max_p=0.25,
                                 params={"limit": 80.0, "asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    # Safety hard constraints (knee / base contacts, foot force, front HFE range, roll-over)
    contact = ConstraintTerm(func=constraints.contact, max_p=1.0,
                             params={"asset_cfg": SceneEntityCfg("contact_forces",
                                                                 body_names=["base_link", ".*_UPPER_LEG"])})
    foot_contact_force = ConstraintTerm(func=constraints.foot_contact_force, max_p=1.0,
                                        params={"limit": 50.0,
                                                "asset_cfg": SceneEntityCfg("contact_forces", body_names=".*_FOOT")})
    front_hfe_position = ConstraintTerm(func=constraints.joint_position, max_p=1.0,
                                        params={"limit": 1.3,
                                                "asset_cfg": SceneEntityCfg("robot", joint_names=["FL_HFE", "FR_HFE"])})
    upsidedown = ConstraintTerm(func=constraints.upsidedown, max_p=1.0,
                                params={"limit": 0.0, "asset_cfg": SceneEntityCfg("robot")})
    # Style constraints
    hip_position = ConstraintTerm(func=constraints.joint_position_when_moving_forward, max_p=0.25,
                                  params={"limit": 0.2, "velocity_deadzone": 0.1,
                                          "asset_cfg": SceneEntityCfg("robot", joint_names=[".*_HAA"])})
    base_orientation = ConstraintTerm(func=constraints.base_orientation, max_p=0.25,
                                      params={"limit": 0.1, "asset_cfg": SceneEntityCfg("robot")})
    air_time = ConstraintTerm(func=constraints.air_time, max_p=0.25,
                              params={"limit": 0.25, "velocity_deadzone": 0.1,
                                      "asset_cfg": SceneEntityCfg("contact_forces", body_names=".*_FOOT")})
    no_move = ConstraintTerm(func=constraints.no_move, max_p=0.1,
                             params={"velocity_deadzone": 0.1, "joint_vel_limit": 4.0,
                                     "asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    two_foot_contact = ConstraintTerm(func=constraints.n_foot_contact, max_p=0.25,
                                      params={"number_of_desired_feet": 2, "min_command_value": 0.5,
                                              "asset_cfg": SceneEntityCfg("contact_forces", body_names=".*_FOOT")})


@configclass
class SixConstraintsCfg:
    """BASELINE.json config 2: six terms, 42 columns (C3, C4, C7, C13, C12, C8)."""
    joint_torque = ConstraintsCfg.__dataclass_fields__["joint_torque"].default_factory()
    joint_velocity = ConstraintsCfg.__dataclass_fields__["joint_velocity"].default_factory()
    contact = ConstraintsCfg.__dataclass_fields__["contact"].default_factory()
    foot_contact_force = ConstraintsCfg.__dataclass_fields__["foot_contact_force"].default_factory()
    action_rate = ConstraintsCfg.__dataclass_fields__["action_rate"].default_factory()
    base_orientation = ConstraintsCfg.__dataclass_fields__["base_orientation"].default_factory()


@configclass
class TwoConstraintsCfg:
    """BASELINE.json config 1 (plumbing case): two terms, 13 columns - one soft (C3 joint_torque), one hard
    boolean (C7 contact)."""
    joint_torque = ConstraintsCfg.__dataclass_fields__["joint_torque"].default_factory()
    contact = ConstraintsCfg.__dataclass_fields__["contact"].default_factory()


@configclass
class ThreeConstraintsCfg:
    """the servo learning experiment: one soft safety, one hard safety and one style term.  (With all 13 terms and the
    initial action noise of 1 some term is violated in 99.8 % of the env steps, the action-rate term alone in about 97 %.)"""
    joint_torque = ConstraintsCfg.__dataclass_fields__["joint_torque"].default_factory()
    foot_contact_force = ConstraintsCfg.__dataclass_fields__["foot_contact_force"].default_factory()
    base_orientation = ConstraintsCfg.__dataclass_fields__["base_orientation"].default_factory()


MAX_CURRICULUM_ITERATIONS = 1000


def _anneal(term_name: str) -> CurrTerm:
    return CurrTerm(func=curriculums.modify_constraint_p,
                    params={"term_name": term_name, "num_steps": 24 * MAX_CURRICULUM_ITERATIONS, "init_max_p": 0.25})


@configclass
class CurriculumCfg:
    # soft safety constraints
    joint_torque = _anneal("joint_torque")
    joint_velocity = _anneal("joint_velocity")
    joint_acceleration = _anneal("joint_acceleration")
    action_rate = _anneal("action_rate")
    # style constraints
    hip_position = _anneal("hip_position")
    base_orientation = _anneal("base_orientation")
    air_time = _anneal("air_time")
    two_foot_contact = _anneal("two_foot_contact")


@configclass
class SixCurriculumCfg:
    joint_torque = _anneal("joint_torque")
    joint_velocity = _anneal("joint_velocity")
    action_rate = _anneal("action_rate")
    base_orientation = _anneal("base_orientation")


@configclass
class TwoCurriculumCfg:
    joint_torque = _anneal("joint_torque")


@configclass
class ThreeCurriculumCfg:
    joint_torque = _anneal("joint_torque")
    base_orientation = _anneal("base_orientation")


@configclass
class SceneCfg:
    num_envs: int = 4096
    env_spacing: float = 3.0
    env_offset: int = 0          # global id of this process's first env (env-sharded runs of the servo simulator)
    robot: object = None         # an ArticulationCfg: its actuators are evaluated inside the servo simulator's launch


@configclass
class SimCfg:
    dt: float = 0.005
    device: str = "cuda:0"


@configclass
class SyntheticCfg:
    """stand-in for Isaac Sim: seeded streams of sim state / reward / resets / observations"""
    obs_dim: int = 45            # ang_vel 3 + cmd 3 + gravity 3 + joint_pos 12 + joint_vel 12 + last_action 12
    stream_steps: int = 48       # stream length (cycled)
    seed_offset: int = 1234
    exact_reset_sync: bool = False
    # "stream": the pre-generated open-loop streams above.  "servo": the closed-loop Solo12 servo surrogate
    # (csrc/servo_sim.hip), whose state follows the actions; its constants are the servo_* fields.
    kind: str = "stream"
    servo_kp: float = 3.0                # joint servo: tau = clamp(kp (q_des - q) - kd qd, +-tau_max), qdd = tau / inertia
    servo_kd: float = 0.2
    servo_inertia: float = 0.004
    servo_tau_max: float = 3.5
    servo_action_scale: float = 0.5      # q_des = default_joint_pos + action_scale * action
    servo_vel_alpha: float = 0.5         # base velocity lag per control step
    servo_tilt_beta: float = 0.3         # roll / pitch lag per control step
    servo_tilt_max: float = 0.35         # |(roll, pitch)| beyond which the robot has rolled over (hard reset)
    servo_reward_scale: float = 0.25     # s of the rational tracking rewards
    servo_foot_clearance: float = 0.1    # foot clearance [m] per rad of knee flexion
    servo_contact_threshold: float = 0.02
    servo_stand_height: float = 0.25     # hip height of a leg at the default pose
    servo_height_drop: float = 0.2       # hip height lost per rad of HFE offset
    servo_floor_height: float = 0.05     # base height with no stance leg
    servo_min_height: float = 0.12       # below it the base body touches the ground
    servo_base_stiffness: float = 200.0  # base contact force [N] per m below servo_min_height
    servo_weight: float = 25.0           # shared between the stance feet
    servo_impact_gain: float = 8.0       # touch-down impulse [N] per rad/s of knee velocity
    servo_init_noise: float = 0.1        # width of the uniform joint noise of an episode's first pose
    # the built-in command generator; with cfg.commands (a CommandsCfg) the simulator runs that command term instead and
    # these three fields are unused
    servo_resample_steps: int = 250      # a new command every so many control steps
    servo_standing_fraction: float = 0.02
    servo_command_deadzone: float = 0.1


@configclass
class Solo12FlatEnvCfg:
    scene: SceneCfg = SceneCfg(num_envs=4096, env_spacing=3.0)
    sim: SimCfg = SimCfg()
    constraints: ConstraintsCfg = ConstraintsCfg()
    curriculum: CurriculumCfg = CurriculumCfg()
    synthetic: SyntheticCfg = SyntheticCfg()
    decimation: int = 4
    episode_length_s: float = 10.0
    seed: int = 42


@configclass
class Solo12ServoFlatEnvCfg(Solo12FlatEnvCfg):
    """the same task on the closed-loop servo surrogate: rewards, observations and constraints follow the actions"""
    synthetic: SyntheticCfg = SyntheticCfg(kind="servo")


@configclass
class Solo12ServoFlatEnvCfg_PLAY(Solo12ServoFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None


@configclass
class RewardsCfg:
    """the reference's reward block (solo12/cat_flat_env_cfg.py RewardsCfg): the two exp tracking terms"""
    track_lin_vel_xy_exp = RewTerm(func=rewards.track_lin_vel_xy_exp, weight=1.0,
                                   params={"command_name": "base_velocity", "std": math.sqrt(0.25)})
    track_ang_vel_z_exp = RewTerm(func=rewards.track_ang_vel_z_exp, weight=0.5,
                                  params={"command_name": "base_velocity", "std": math.sqrt(0.25)})


@configclass
class ShapedRewardsCfg:
    """``RewardsCfg`` plus a few of the penalties people add first (IsaacLab's velocity-task magnitudes)"""
    track_lin_vel_xy_exp = RewardsCfg.__dataclass_fields__["track_lin_vel_xy_exp"].default_factory()
    track_ang_vel_z_exp = RewardsCfg.__dataclass_fields__["track_ang_vel_z_exp"].default_factory()
    ang_vel_xy_l2 = RewTerm(func=rewards.ang_vel_xy_l2, weight=-0.05)
    flat_orientation_l2 = RewTerm(func=rewards.flat_orientation_l2, weight=-1.0)
    joint_torques_l2 = RewTerm(func=rewards.joint_torques_l2, weight=-1.0e-4,
                               params={"asset_cfg": SceneEntityCfg("robot", joint_names=ALL_JOINTS)})
    action_rate_l2 = RewTerm(func=rewards.action_rate_l2, weight=-0.01)
    hip_deviation = RewTerm(func=rewards.joint_deviation_l1, weight=-0.1,
                            params={"asset_cfg": SceneEntityCfg("robot", joint_names=[".*_HAA"])})
    feet_air_time = RewTerm(func=rewards.feet_air_time, weight=0.25,
                            params={"command_name": "base_velocity", "threshold": 0.25,
                                    "sensor_cfg": SceneEntityCfg("contact_forces", body_names=".*_FOOT")})
    is_terminated = RewTerm(func=rewards.is_terminated, weight=-20.0)


@configclass
class Solo12ServoRewardsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable reward block: the simulator's launch evaluates ``rewards`` term by term"""
    rewards: RewardsCfg = RewardsCfg()


@configclass
class Solo12ServoRewardsFlatEnvCfg_PLAY(Solo12ServoRewardsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None


# the reference observes the joints in this order (hind right before hind left), by name
OBS_JOINTS = ["FL_HAA", "FL_HFE", "FL_KFE", "FR_HAA", "FR_HFE", "FR_KFE", "HR_HAA", "HR_HFE", "HR_KFE", "HL_HAA", "HL_HFE", "HL_KFE"]


@configclass
class ObservationsCfg:
    """the reference's observation block (solo12/cat_flat_env_cfg.py ObservationsCfg): six terms, 45 floats"""

    @configclass
    class PolicyCfg(ObsGroup):
        base_ang_vel = ObsTerm(func=observations.base_ang_vel, noise=Unoise(n_min=-0.001, n_max=0.001), scale=0.25)
        velocity_commands = ObsTerm(func=observations.generated_commands, params={"command_name": "base_velocity"},
                                    scale=(2.0, 2.0, 0.25))
        projected_gravity = ObsTerm(func=observations.projected_gravity, noise=Unoise(n_min=-0.05, n_max=0.05), scale=0.1)
        joint_pos = ObsTerm(func=observations.joint_pos, noise=Unoise(n_min=-0.01, n_max=0.01), scale=1.0,
                            params={"asset_cfg": SceneEntityCfg("robot", joint_names=OBS_JOINTS, preserve_order=True)})
        joint_vel = ObsTerm(func=observations.joint_vel, noise=Unoise(n_min=-0.2, n_max=0.2), scale=0.05,
                            params={"asset_cfg": SceneEntityCfg("robot", joint_names=OBS_JOINTS, preserve_order=True)})
        actions = ObsTerm(func=observations.last_action, scale=1.0)
        enable_corruption: bool = True
        concatenate_terms: bool = True

    policy: PolicyCfg = PolicyCfg()


@configclass
class Solo12ServoObsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable observation block: the simulator's launch evaluates ``observations`` term by term"""
    observations: ObservationsCfg = ObservationsCfg()


@configclass
class Solo12ServoObsFlatEnvCfg_PLAY(Solo12ServoObsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None

    def __post_init__(self):
        self.observations.policy.enable_corruption = False


@configclass
class EventCfg:
    """the reference's event block (solo12/cat_flat_env_cfg.py EventCfg): traction at start-up, two reset terms, the push"""
    physics_material = EventTerm(func=events.randomize_rigid_body_material, mode="startup",
                                 params={"asset_cfg": SceneEntityCfg("robot", body_names=".*"),
                                         "static_friction_range": (0.5, 1.25), "dynamic_friction_range": (0.5, 1.25),
                                         "restitution_range": (0.0, 0.0), "num_buckets": 100})
    reset_base = EventTerm(func=events.reset_root_state_uniform, mode="reset",
                           params={"pose_range": {"x": (-0.05, 0.05), "y": (-0.05, 0.05), "yaw": (-1.57, 1.57)},
                                   "velocity_range": {"x": (-0.0, 0.0), "y": (-0.0, 0.0), "z": (-0.0, 0.0),
                                                      "roll": (-0.0, 0.0), "pitch": (-0.0, 0.0), "yaw": (-0.0, 0.0)}})
    reset_robot_joints = EventTerm(func=events.reset_joints_by_scale, mode="reset",
                                   params={"position_range": (0.95, 1.05), "velocity_range": (-0.05, 0.05)})
    # every step, each env with probability physics_dt / (2 * max_episode_length_s)
    push_robot = EventTerm(func=events.push_by_setting_velocity_with_random_envs, mode="interval", is_global_time=True,
                           interval_range_s=(0.0, 0.005),
                           params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})


@configclass
class Solo12ServoEventsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable event block: the simulator's launch evaluates ``events`` term by term"""
    events: EventCfg = EventCfg()


@configclass
class Solo12ServoEventsFlatEnvCfg_PLAY(Solo12ServoEventsFlatEnvCfg):
    """reset and startup terms stay (they define the task); the env runs with pushes off (``event_manager``)"""
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None
    pushes: bool = False


@configclass
class Solo12ServoFullFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """rewards, observations and events together: the reference's whole MDP block on the surrogate"""
    rewards: RewardsCfg = RewardsCfg()
    observations: ObservationsCfg = ObservationsCfg()
    events: EventCfg = EventCfg()


@configclass
class Solo12ServoFullFlatEnvCfg_PLAY(Solo12ServoFullFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None
    pushes: bool = False

    def __post_init__(self):
        self.observations.policy.enable_corruption = False


@configclass
class CommandsCfg:
    """the reference's command block (solo12/cat_flat_env_cfg.py CommandsCfg): one velocity command with a dead zone"""
    base_velocity = commands.UniformVelocityCommandWithDeadzoneCfg(
        asset_name="robot", resampling_time_range=(10.0, 10.0), rel_standing_envs=0.02, rel_heading_envs=1.0,
        heading_command=False, debug_vis=True, velocity_deadzone=0.1,
        ranges=commands.UniformVelocityCommandCfg.Ranges(lin_vel_x=(-0.3, 1.0), lin_vel_y=(-0.7, 0.7), ang_vel_z=(-0.78, 0.78)))


@configclass
class Solo12ServoCommandsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable command block: the simulator's launch runs ``commands``' velocity command term"""
    commands: CommandsCfg = CommandsCfg()


@configclass
class Solo12ServoCommandsFlatEnvCfg_PLAY(Solo12ServoCommandsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None


@configclass
class Solo12ServoReferenceFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """rewards, observations, events and commands: the four configurable parts of the reference's MDP block together"""
    rewards: RewardsCfg = RewardsCfg()
    observations: ObservationsCfg = ObservationsCfg()
    events: EventCfg = EventCfg()
    commands: CommandsCfg = CommandsCfg()


@configclass
class Solo12ServoReferenceFlatEnvCfg_PLAY(Solo12ServoReferenceFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None
    pushes: bool = False

    def __post_init__(self):
        self.observations.policy.enable_corruption = False


@configclass
class TerminationsCfg:
    """the reference's termination block (solo12/cat_flat_env_cfg.py TerminationsCfg): three terms and their values"""
    time_out = DoneTerm(func=terminations.time_out, time_out=True)
    base_contact = DoneTerm(func=terminations.illegal_contact,
                            params={"sensor_cfg": SceneEntityCfg("contact_forces", body_names=["base_link", ".*_UPPER_LEG"]),
                                    "threshold": 1.0})
    upside_down = DoneTerm(func=terminations.upside_down, params={"limit": 0.1})


@configclass
class BuiltinTerminationsCfg:
    """what ends an episode of the servo task without a termination block, said as one: the time-out and the roll-over flag"""
    time_out = DoneTerm(func=terminations.time_out, time_out=True)
    rolled_over = DoneTerm(func=terminations.rolled_over)


@configclass
class Solo12ServoTerminationsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable termination block: the simulator's launch evaluates ``terminations``' terms"""
    terminations: TerminationsCfg = TerminationsCfg()


@configclass
class Solo12ServoTerminationsFlatEnvCfg_PLAY(Solo12ServoTerminationsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None


@configclass
class Solo12ServoReferenceTerminationsFlatEnvCfg(Solo12ServoReferenceFlatEnvCfg):
    """rewards, observations, events, commands and terminations: five of the six MDP blocks of the reference's cfg (the
    action block is ``Solo12ServoReferenceActionsFlatEnvCfg``'s)"""
    terminations: TerminationsCfg = TerminationsCfg()


@configclass
class Solo12ServoReferenceTerminationsFlatEnvCfg_PLAY(Solo12ServoReferenceFlatEnvCfg_PLAY):
    terminations: TerminationsCfg = TerminationsCfg()


@configclass
class ActionsCfg:
    """the reference's action block (solo12/cat_flat_env_cfg.py ActionsCfg): one joint position term over all twelve joints
    in the reference's order FL FR HR HL (the simulator's joints are FL FR HL HR), scale 0.5, offset = the default pose"""
    joint_pos = actions.JointPositionActionCfg(asset_name="robot", joint_names=OBS_JOINTS, scale=0.5, use_default_offset=True,
                                               preserve_order=True)


@configclass
class Solo12ServoActionsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with a configurable action block: the simulator's launch evaluates ``actions``' terms"""
    actions: ActionsCfg = ActionsCfg()


@configclass
class Solo12ServoActionsFlatEnvCfg_PLAY(Solo12ServoActionsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None


@configclass
class Solo12ServoReferenceActionsFlatEnvCfg(Solo12ServoReferenceTerminationsFlatEnvCfg):
    """rewards, observations, events, commands, terminations and actions: every MDP block of the reference's cfg"""
    actions: ActionsCfg = ActionsCfg()


@configclass
class Solo12ServoReferenceActionsFlatEnvCfg_PLAY(Solo12ServoReferenceTerminationsFlatEnvCfg_PLAY):
    actions: ActionsCfg = ActionsCfg()


def _delayed(robot, min_delay, max_delay):
    """``robot`` with every actuator group turned into a ``DelayedPDActuatorCfg`` of the same joints, gains and limits"""
    fields = ("joint_names_expr", "effort_limit", "velocity_limit", "stiffness", "damping", "armature", "friction")
    return robot.replace(actuators={n: DelayedPDActuatorCfg(**{f: getattr(a, f) for f in fields}, min_delay=min_delay,
                                                            max_delay=max_delay) for n, a in robot.actuators.items()})


@configclass
class Solo12ServoActuatorsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with the reference's robot: the simulator's launch evaluates its actuators"""
    scene: SceneCfg = SceneCfg(num_envs=4096, env_spacing=3.0, robot=SOLO12_MINIMAL_CFG)


@configclass
class Solo12ServoActuatorsFlatEnvCfg_PLAY(Solo12ServoActuatorsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0, robot=SOLO12_MINIMAL_CFG)
    curriculum: object = None


@configclass
class Solo12ServoReferenceActuatorsFlatEnvCfg(Solo12ServoReferenceActionsFlatEnvCfg):
    """every MDP block of the reference's cfg and the reference's robot"""
    scene: SceneCfg = SceneCfg(num_envs=4096, env_spacing=3.0, robot=SOLO12_MINIMAL_CFG)


@configclass
class Solo12ServoReferenceActuatorsFlatEnvCfg_PLAY(Solo12ServoReferenceActionsFlatEnvCfg_PLAY):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0, robot=SOLO12_MINIMAL_CFG)


@configclass
class Solo12ServoDelayedActuatorsFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the reference's gains behind an actuator delay of 0 .. 4 physics steps (up to one control step), drawn per episode"""
    scene: SceneCfg = SceneCfg(num_envs=4096, env_spacing=3.0, robot=_delayed(SOLO12_MINIMAL_CFG, 0, 4))


@configclass
class Solo12ServoDelayedActuatorsFlatEnvCfg_PLAY(Solo12ServoDelayedActuatorsFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0, robot=_delayed(SOLO12_MINIMAL_CFG, 0, 4))
    curriculum: object = None


def _randomization_terms():
    """this project's choice of ranges (the reference randomises none of the three): gains +- 20 % per env, a joint friction
    of up to 0.05 N m per episode, -0.5 .. +1 kg on the base per env"""
    return dict(
        actuator_gains=EventTerm(func=events.randomize_actuator_gains, mode="startup",
                                 params={"asset_cfg": SceneEntityCfg("robot", joint_names=".*"),
                                         "stiffness_distribution_params": (0.8, 1.2),
                                         "damping_distribution_params": (0.8, 1.2), "operation": "scale",
                                         "distribution": "uniform"}),
        joint_parameters=EventTerm(func=events.randomize_joint_parameters, mode="reset",
                                   params={"asset_cfg": SceneEntityCfg("robot", joint_names=".*"),
                                           "friction_distribution_params": (0.0, 0.05), "operation": "abs",
                                           "distribution": "uniform"}),
        add_base_mass=EventTerm(func=events.randomize_rigid_body_mass, mode="startup",
                                params={"asset_cfg": SceneEntityCfg("robot", body_names="base_link"),
                                        "mass_distribution_params": (-0.5, 1.0), "operation": "add"}))


@configclass
class RandomizationEventCfg:
    """the robot of every env is its own ("Randomisation"): gains, joint friction and base mass"""
    actuator_gains = _randomization_terms()["actuator_gains"]
    joint_parameters = _randomization_terms()["joint_parameters"]
    add_base_mass = _randomization_terms()["add_base_mass"]


@configclass
class ReferenceRandomizationEventCfg(EventCfg):
    """the reference's event block with the three randomisation terms added"""
    actuator_gains = _randomization_terms()["actuator_gains"]
    joint_parameters = _randomization_terms()["joint_parameters"]
    add_base_mass = _randomization_terms()["add_base_mass"]


@configclass
class Solo12ServoRandomizedFlatEnvCfg(Solo12ServoActuatorsFlatEnvCfg):
    """the servo task with the reference's robot, randomised per env: an event block of randomisation terms alone"""
    events: RandomizationEventCfg = RandomizationEventCfg()


@configclass
class Solo12ServoRandomizedFlatEnvCfg_PLAY(Solo12ServoActuatorsFlatEnvCfg_PLAY):
    """randomisation stays on, pushes (there are none) off"""
    events: RandomizationEventCfg = RandomizationEventCfg()
    pushes: bool = False


@configclass
class Solo12ServoReferenceRandomizedFlatEnvCfg(Solo12ServoReferenceActuatorsFlatEnvCfg):
    """every MDP block of the reference's cfg, the reference's robot and the three randomisation terms"""
    events: ReferenceRandomizationEventCfg = ReferenceRandomizationEventCfg()


@configclass
class Solo12ServoReferenceRandomizedFlatEnvCfg_PLAY(Solo12ServoReferenceActuatorsFlatEnvCfg_PLAY):
    """randomisation stays on, pushes off"""
    events: ReferenceRandomizationEventCfg = ReferenceRandomizationEventCfg()


@configclass
class DisturbanceEventCfg(EventCfg):
    """the reference's event block with IsaacLab's stock disturbances ("Disturbances"): the push on a timer of
    the env's own, and a constant external force on the base per episode"""
    # IsaacLab's velocity task pushes every 10 .. 15 s; an episode here is 10 s long, so that timer would fire at most once per
    # episode and in most episodes never: 2 .. 4 s gives two to four pushes per episode
    push_robot = EventTerm(func=events.push_by_setting_velocity, mode="interval", interval_range_s=(2.0, 4.0),
                           params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}})
    # IsaacLab's stock term has both ranges (0, 0); up to an eighth of the robot's weight, in every direction
    base_external_force_torque = EventTerm(func=events.apply_external_force_torque, mode="reset",
                                           params={"asset_cfg": SceneEntityCfg("robot", body_names="base_link"),
                                                   "force_range": (-3.0, 3.0), "torque_range": (-0.3, 0.3)})


@configclass
class Solo12ServoDisturbancesFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task under timed pushes and an external wrench: the simulator's launch evaluates both"""
    events: DisturbanceEventCfg = DisturbanceEventCfg()


@configclass
class Solo12ServoDisturbancesFlatEnvCfg_PLAY(Solo12ServoDisturbancesFlatEnvCfg):
    """reset and startup terms and the wrench stay; the env runs with pushes off"""
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None
    pushes: bool = False


@configclass
class Solo12ServoReferenceDisturbancesFlatEnvCfg(Solo12ServoReferenceActuatorsFlatEnvCfg):
    """every MDP block of the reference's cfg and the reference's robot, under timed pushes and an external wrench"""
    events: DisturbanceEventCfg = DisturbanceEventCfg()


@configclass
class Solo12ServoReferenceDisturbancesFlatEnvCfg_PLAY(Solo12ServoReferenceActuatorsFlatEnvCfg_PLAY):
    """the wrench stays on, pushes off (inherited)"""
    events: DisturbanceEventCfg = DisturbanceEventCfg()


@configclass
class HistoryObservationsCfg:
    """the reference's six terms, each with its last three processed frames, oldest first ("History"): 135 floats"""

    @configclass
    class PolicyCfg(ObservationsCfg.PolicyCfg):
        history_length: int = 3

    policy: PolicyCfg = PolicyCfg()


@configclass
class Solo12ServoHistoryFlatEnvCfg(Solo12ServoFlatEnvCfg):
    """the servo task with an observation history: the simulator's launch keeps the last three frames of every term in its row"""
    observations: HistoryObservationsCfg = HistoryObservationsCfg()


@configclass
class Solo12ServoHistoryFlatEnvCfg_PLAY(Solo12ServoHistoryFlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None

    def __post_init__(self):
        self.observations.policy.enable_corruption = False


@configclass
class Solo12ServoReferenceHistoryFlatEnvCfg(Solo12ServoReferenceRandomizedFlatEnvCfg):
    """every MDP block of the reference's cfg, the reference's robot behind an actuator delay, the three randomisation terms,
    and three frames of every observation term: what lets a policy tell the delayed, randomised robots apart"""
    scene: SceneCfg = SceneCfg(num_envs=4096, env_spacing=3.0, robot=_delayed(SOLO12_MINIMAL_CFG, 0, 4))
    observations: HistoryObservationsCfg = HistoryObservationsCfg()


@configclass
class Solo12ServoReferenceHistoryFlatEnvCfg_PLAY(Solo12ServoReferenceRandomizedFlatEnvCfg_PLAY):
    """randomisation stays on, pushes and observation noise off (the inherited ``__post_init__``)"""
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0, robot=_delayed(SOLO12_MINIMAL_CFG, 0, 4))
    observations: HistoryObservationsCfg = HistoryObservationsCfg()


@configclass
class Solo12FlatEnvCfg_PLAY(Solo12FlatEnvCfg):
    scene: SceneCfg = SceneCfg(num_envs=50, env_spacing=3.0)
    curriculum: object = None
