"""windgym_amd — MI355X-native batched implementation of WindGym's step() transition.

Public names mirror the reference package (WindGym/__init__.py): ``WindFarmEnv``, ``FarmEval``,
``WindFarmEnvMulti``; plus the native batched ``WindFarmVecEnv`` / ``WindFarmVecEnvMulti`` and the ``V80`` tabular turbine.
"""
from .turbine import V80, TabularTurbine  # noqa: F401
from .config import EnvConfig  # noqa: F401


def __getattr__(name):   # lazy: importing the env classes pulls in torch
    if name in ("WindFarmEnv", "FarmEval", "WindFarmEnvMulti", "WindFarmVecEnv", "WindFarmVecEnvMulti", "RecordEpisodeVals"):
        from . import envs
        return getattr(envs, name)
    if name == "HipBatch":
        from .binding import HipBatch
        return HipBatch
    if name in ("AgentEval", "eval_sweep"):
        from . import evaluate
        return getattr(evaluate, name)
    if name in ("ConstantAgent", "RandomAgent", "GreedyAgent", "BaseAgent"):
        from . import agents
        return getattr(agents, name)
    if name in ("MlpPolicy", "read_sb3_zip"):
        from . import policy
        return getattr(policy, name)
    if name in ("MlpLstmPolicy", "read_sb3_lstm_zip"):
        from . import recurrent
        return getattr(recurrent, name)
    if name in ("PPO", "PPOOptimizer"):
        from . import ppo
        return getattr(ppo, name)
    if name in ("RecurrentPPO", "RecurrentPPOOptimizer"):
        from . import recurrent_ppo
        return getattr(recurrent_ppo, name)
    if name in ("PPOPopulation", "Population"):
        from . import population
        return getattr(population, name)
    if name in ("RecurrentPPOPopulation", "RecurrentPopulation"):
        from . import recurrent_population
        return getattr(recurrent_population, name)
    if name == "YawCurriculum":
        from .curriculum import YawCurriculum
        return YawCurriculum
    if name == "BehaviorCloning":
        from .imitation import BehaviorCloning
        return BehaviorCloning
    if name == "RecurrentBehaviorCloning":
        from .recurrent_imitation import RecurrentBehaviorCloning
        return RecurrentBehaviorCloning
    if name in ("YawTable", "YawTableAgent"):
        from . import yaw_table
        return getattr(yaw_table, name)
    if name == "VecNormalize":
        from .normalize import VecNormalize
        return VecNormalize
    if name in ("PyWakeAgent", "SteadyStateYawAgent", "PyWakeVecAgent", "SteadyStateYawVecAgent"):
        from . import steady
        return getattr(steady, name)
    raise AttributeError(name)
