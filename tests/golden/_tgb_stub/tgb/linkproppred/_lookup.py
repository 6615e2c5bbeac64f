"""What the three stand-in samplers share: a dict evaluation set per split and a lookup."""
import numpy as np


def as_list(v):
    """A batch vector (torch tensor, numpy array, list) as Python integers."""
    if hasattr(v, 'detach'):
        v = v.detach().cpu().numpy()
    return np.asarray(v).reshape(-1).tolist()


class LookupSampler:
    def __init__(self, dataset_name):
        self.dataset_name = dataset_name
        self.eval_set = {}

    def load_eval_set(self, fname, split_mode='val'):
        if split_mode not in ('val', 'test'):
            raise ValueError(f'Invalid split-mode: {split_mode}')
        self.eval_set.setdefault(split_mode, {})

    def _lookup(self, keys, split_mode):
        table = self.eval_set[split_mode]
        out = []
        for key in keys:
            if key not in table:
                raise ValueError(f'The edge {key} is not in the {split_mode} evaluation set of {self.dataset_name}')
            out.append([int(x) for x in table[key]])
        return out
