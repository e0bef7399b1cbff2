"""The reference's plugin registries with the same keys (utils/name_match.py:31-55), restricted to the hot path
BASELINE.json names.  `general_main.py` of the reference becomes a drop-in by importing these dictionaries
instead of its own."""


class _Lazy(dict):
    """Registry whose values are resolved on first access (avoids import cycles: Buffer -> name_match -> plugins)."""

    def __init__(self, table):
        super().__init__()
        self._table = table

    def __missing__(self, key):
        if key not in self._table:
            raise KeyError(key)
        mod, attr = self._table[key]
        import importlib
        val = getattr(importlib.import_module(mod, __package__), attr)
        self[key] = val
        return val

    def __contains__(self, key):
        return key in self._table

    def keys(self):
        return self._table.keys()


agents = _Lazy({
    'ER': ('.agents.exp_replay', 'ExperienceReplay'),
    'SCR': ('.agents.scr', 'SupContrastReplay'),
})

# agents beyond the BASELINE hot path (`agents` keeps the keys INTEGRATION.md section 1 moves; these are added by name, section 1b)
extra_agents = _Lazy({
    'AGEM': ('.agents.agem', 'AGEM'),
})


# regularisation-based agents: no replay memory, their bookkeeping runs on the flat parameter and gradient arrays (section 1b as well)
regularization_agents = _Lazy({
    'EWC': ('.agents.ewc_pp', 'EWC_pp'),
})


# regularisation by distillation against last task's model: no replay memory either; the teacher is KdManager's parameter snapshot
# (section 1b as well; a table of its own because tests/test_cpu_ewc.py pins `regularization_agents` to EWC alone)
distillation_agents = _Lazy({
    'LWF': ('.agents.lwf', 'Lwf'),
})


# agents that train offline on their memory at every task's end (section 1b as well)
offline_agents = _Lazy({
    'GDUMB': ('.agents.gdumb', 'Gdumb'),
})


# agents that replay exemplars against a distilled target and classify by the nearest class mean (section 1b as well; a table of its
# own because every table above is pinned to its keys by a test)
exemplar_agents = _Lazy({
    'ICARL': ('.agents.icarl', 'Icarl'),
})


# agents that replay stored logits beside the labels (Dark Experience Replay; an addition beyond the reference's registry; section 1b
# as well, and a table of its own for the same reason)
logit_replay_agents = _Lazy({
    'DER': ('.agents.der', 'Der'),
})


def get_agent(key):
    """The agent class registered under `key`: `agents` first, then `extra_agents`, `regularization_agents`, `distillation_agents`,
    `offline_agents`, `exemplar_agents` and `logit_replay_agents`; KeyError otherwise."""
    for table in (agents, extra_agents, regularization_agents, distillation_agents, offline_agents, exemplar_agents, logit_replay_agents):
        if key in table:
            return table[key]
    raise KeyError(key)


retrieve_methods = _Lazy({
    'MIR': ('.plugins.mir_retrieve', 'MIR_retrieve'),
    'random': ('.plugins.random_retrieve', 'Random_retrieve'),
    'ASER': ('.plugins.aser_retrieve', 'ASER_retrieve'),
    'match': ('.plugins.sc_retrieve', 'Match_retrieve'),
    'mem_match': ('.plugins.mem_match', 'MemMatch_retrieve'),
})

update_methods = _Lazy({
    'random': ('.plugins.reservoir_update', 'Reservoir_update'),
    'GSS': ('.plugins.gss_greedy_update', 'GSSGreedyUpdate'),
    'ASER': ('.plugins.aser_update', 'ASER_update'),
})
