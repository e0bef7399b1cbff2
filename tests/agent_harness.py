"""What the agents' GPU tests share: the parameters and construction of an agent for a case of oracle.synth, the host RNG streams
saved / restored / compared, and small tensor helpers.  A plain module (no fixtures): `from agent_harness import build_agent, ...`."""
import random
from types import SimpleNamespace

import numpy as np
import torch

from guarded import _bits
from oracle.synth import case_params, seed_all

TRICK = {'labels_trick': False, 'kd_trick': False, 'separated_softmax': False, 'review_trick': False, 'ncm_trick': False,
         'kd_trick_star': False}


def make_params(cfg, *, extra=None, **over):
    """The agent's params: the defaults below, then the case's own (case_params), then `extra` (what an agent's *_ref module adds to
    them: a dict, or a function of the case that returns one, such as ewc_ref.ref_params), then the caller's overrides."""
    p = dict(agent="ER", retrieve="random", update="random", data="cifar100", mem_size=1000, eps_mem_batch=10, cuda=True, epoch=1,
             batch=10, test_batch=128, verbose=False, optimizer="SGD", learning_rate=0.1, weight_decay=0, mem_iters=1, subsample=50, k=3,
             aser_type="asvm", n_smp_cls=1.5, num_tasks=10, temp=0.07, head="mlp", buffer_tracker=False, error_analysis=False, seed=0,
             trick=dict(TRICK))
    p.update(case_params(cfg))
    p.update((extra(cfg) if callable(extra) else extra) or {})
    p.update(over)
    return SimpleNamespace(**p)


def build_agent(cfg, *, extra=None, **over):
    """-> (params, model, opt, agent), seeded with the case's seed; the agent is the one `agent` names in `over` or in the case."""
    from ocl_amd import name_match
    from ocl_amd.setup_elements import setup_architecture, setup_opt
    from ocl_amd.utils import maybe_cuda
    params = make_params(cfg, extra=extra, **over)
    seed_all(cfg["seed"])
    model = maybe_cuda(setup_architecture(params), params.cuda)
    opt = setup_opt(params.optimizer, model, params.learning_rate, params.weight_decay)
    agent = name_match.get_agent(params.agent)(model, opt, params)
    if params.agent == "SCR":
        agent.transform = lambda x: x      # identity augmentation on both sides (kornia is unpinned)
    return params, model, opt, agent


# ---- the host RNG streams: torch's and numpy's, with python=True also `random`'s (GDumb's balancer draws from it) --------------------------

def rng_get(python=False):
    return (torch.get_rng_state(), np.random.get_state()) + ((random.getstate(),) if python else ())


def rng_set(st):
    torch.set_rng_state(st[0])
    np.random.set_state(st[1])
    if len(st) > 2:
        random.setstate(st[2])


def rng_equal(a, b):
    return (torch.equal(a[0], b[0]) and all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a[1], b[1]))
            and a[2:] == b[2:])


# ---- tensors ------------------------------------------------------------------------------------------------------------------------------

def flat(state, names):
    return torch.cat([state[k].detach().reshape(-1) for k in names]).double().cpu().numpy()


def events(ev, tag):
    return [e for t, e in ev if t == tag]


def dev(a, cuda, dtype=np.float32):
    """A host array on the device (guarded.dev is another thing: a tensor with slack behind it)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(cuda)


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    """The elements' bit patterns, as integers of the same size."""
    return _bits(t.detach().contiguous())
