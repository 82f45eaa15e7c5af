"""Instances and network input with the surface of the reference's mkp_transformer/utils.py (multidimensional knapsack,
price [n] and weight [m, n] with every capacity normalised to 1)."""
import numpy as np

import torch


def gen_instance(n, m=2, device='cpu'):
    """*Well-stated* instances (mkp_transformer/utils.py:5-22): U(0,1) prices [n] and weights [m, n]; per constraint a
    capacity drawn with numpy (never seeded by the reference: its datasets are not reproducible from torch's seed) between
    the largest single weight and the total weight; weights divided by it, so every capacity is 1."""
    price = torch.rand(size=(n,), device=device)
    weight = torch.rand(size=(m, n), device=device)
    heaviest, _ = torch.max(weight, dim=1)
    total = torch.sum(weight, dim=1)
    caps = [np.random.uniform(low=heaviest[j].item(), high=total[j].item()) for j in range(m)]
    return price, weight / torch.tensor(caps, device=device).unsqueeze(1)


def reformat(price, weight):
    """Network input [n, 1, m+1]: per item its price, then its m weights (mkp_transformer/utils.py:24-30)."""
    return torch.cat((price.unsqueeze(1), weight.T), dim=1).unsqueeze(1)


def _load(path, device):
    dataset = torch.load(path, map_location=device)
    return [(inst[0], inst[1:]) for inst in dataset]


def load_val_dataset(problem_size, device):
    """[(price [n], weight [m, n])] from ./data/mkp_transformer/valDataset-<n>.pt (row 0 = price, the rest = weights)."""
    return _load(f'./data/mkp_transformer/valDataset-{problem_size}.pt', device)


def load_test_dataset(problem_size, device):
    return _load(f'./data/mkp_transformer/testDataset-{problem_size}.pt', device)


if __name__ == "__main__":      # writes ../data/mkp_transformer/* as the reference's utils.py does when run as a script
    import os
    import sys
    try:
        from deepaco_amd.datasets import write_datasets
    except ImportError:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        from deepaco_amd.datasets import write_datasets
    print("\n".join(write_datasets("mkp_transformer", sys.modules[__name__])))
