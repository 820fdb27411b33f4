"""Objectives of the BOCF loop: `MultiObjective`, with the constructor of the reference's multi-output objective and the same use of
np.random (one normal draw per output for a noisy evaluation).  Host code: the objective is the user's simulator.

Results follow GPyOpt's objective convention: `evaluate(X)` returns (list of m column arrays (n, 1), cost)."""
import time

import numpy as np


def _column_by_rows(f, X):
    """f applied to every row of X as a (1, d) array, results stacked into an (n, 1) column; also the wall time of every call."""
    values, seconds = [], []
    for x in np.atleast_2d(X):
        t0 = time.time()
        values.append(np.reshape(f(x[None, :]), (1, 1)))
        seconds.append(time.time() - t0)
    return (np.concatenate(values, 0) if values else np.empty((0, 1))), seconds


class MultiObjective(object):
    """m attributes of a composite objective.

    func: a list of m single-output functions f_j((1, d)) -> scalar or (1, 1) (as_list=True, each called row by row), or one function
    F((n, d)) -> (m, n) (as_list=False, output_dim required).  noise_var: per-output observation-noise variances used by
    evaluate_w_noise (None: noiseless)."""

    def __init__(self, func, noise_var=None, objective_name=None, as_list=True, output_dim=None):
        self.func = func
        self.as_list = as_list
        self.output_dim = len(func) if as_list else output_dim
        self.noise_var = noise_var
        self.objective_name = objective_name if objective_name is not None else ['no_name'] * self.output_dim
        self.objective = func

    def _columns(self, X):
        X = np.atleast_2d(X)
        if self.as_list:
            return [_column_by_rows(f, X)[0] for f in self.func]
        F = np.asarray(self.func(X))
        return [F[j].reshape(X.shape[0], 1) for j in range(self.output_dim)]

    def evaluate(self, X):
        """Noiseless values at the rows of X: (list of m (n, 1) arrays, 0).  Draws nothing from np.random."""
        return self._columns(X), 0

    def evaluate_as_array(self, X):
        """The same values as one (m, n) array."""
        return np.stack([c[:, 0] for c in self._columns(X)])

    def evaluate_w_noise(self, X):
        """evaluate(X) plus observation noise: for j = 0, 1, ... in order, ONE draw np.random.normal(scale=sqrt(noise_var[j])) is added
        to every value of output j."""
        cols, cost = self.evaluate(X)
        if self.noise_var is not None:
            cols = [c + np.random.normal(scale=np.sqrt(nv)) for c, nv in zip(cols, self.noise_var)]
        return cols, cost

    def get_output_dim(self):
        return self.output_dim
