from . import actions, commands, events, observations, rewards, terminations  # noqa: F401
from .event_manager import EventManager  # noqa: F401
from .observation_manager import ObservationManager  # noqa: F401
from .reward_manager import RewardManager  # noqa: F401
