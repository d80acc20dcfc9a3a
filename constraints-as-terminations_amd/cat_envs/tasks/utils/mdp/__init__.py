from . import rewards  # noqa: F401
from .reward_manager import RewardManager  # noqa: F401
