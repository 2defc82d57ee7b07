"""Which checkpoints of a training run still need an evaluation, and where the scores go (the reference's
``xmcgan/utils/task_manager.py``; its ``test`` mode polls a training job's checkpoint directory with it).

A run keeps its checkpoints in ``<workdir>/checkpoints-0`` (the reference's ``MultihostCheckpoint(<workdir>/checkpoints)`` appends
the host index; host 0 is the one that is evaluated).  The directory holds ``ckpt-<n>.flax`` files -- ``n`` is the save ordinal --,
the ``TRAIN_DONE`` marker and ``scores.csv``.  The reference lists the checkpoints through TensorFlow's checkpoint manager; here the
``.flax`` files themselves are listed, so a directory written by the reference is read as it is (its TensorFlow files are ignored).
"""
from __future__ import annotations

import csv
import glob
import logging
import os
import re
import time
from typing import Any, Callable, Dict, Iterable, Optional

_log = logging.getLogger(__name__)
_CKPT = re.compile(r"^ckpt-(\d+)(\.flax)?$")
TRAIN_DONE = "TRAIN_DONE"
POLL_SECONDS = 5


def checkpoint_number(path: str) -> int:
    """the number in ``.../ckpt-<n>[.flax]``"""
    m = _CKPT.match(os.path.basename(path))
    if not m:
        raise ValueError(f"not a checkpoint name: {path}")
    return int(m.group(1))


def _key(path: str) -> str:
    """a checkpoint's identity in ``scores.csv``: its path without the ``.flax`` suffix (the reference's rows hold that prefix)"""
    return path[:-5] if path.endswith(".flax") else path


def list_checkpoints(directory: str):
    """paths of the ``ckpt-<n>.flax`` files of ``directory``, sorted by ``n``"""
    found = [p for p in glob.glob(os.path.join(directory, "ckpt-*.flax")) if _CKPT.match(os.path.basename(p))]
    return sorted(found, key=checkpoint_number)


class TaskManager:
    """Checks a model directory repeatedly for checkpoints to evaluate (task_manager.py:70-157).  ``model_dir`` is the
    ``<workdir>/checkpoints`` prefix; ``clock`` / ``sleep`` replace ``time.time`` / ``time.sleep`` (tests)."""

    def __init__(self, model_dir: str, *, clock: Callable[[], float] = time.time, sleep: Callable[[float], None] = time.sleep) -> None:
        self._model_dir = f"{model_dir.rstrip('/')}-0"
        self._clock, self._sleep = clock, sleep

    @property
    def model_dir(self) -> str:
        return self._model_dir

    def mark_training_done(self) -> None:
        os.makedirs(self.model_dir, exist_ok=True)
        with open(os.path.join(self.model_dir, TRAIN_DONE), "w") as f:
            f.write("")

    def is_training_done(self) -> bool:
        return os.path.exists(os.path.join(self.model_dir, TRAIN_DONE))

    def add_eval_result(self, checkpoint_path: str, result_dict: Dict[str, Any], default_value: int = -1) -> None:
        pass

    def _get_checkpoints_with_results(self):
        return set()

    def unevaluated_checkpoints(self, timeout: float = 3600 * 8, num_batched_steps: int = 1,
                                eval_every_steps: Optional[int] = None) -> Iterable[str]:
        """Yields the checkpoints without a result, lowest number first, and keeps looking for new ones until ``timeout``
        seconds have passed without any or training is done.  ``eval_every_steps``: only numbers ``n > num_batched_steps`` with
        ``n % eval_every_steps < num_batched_steps`` (task_manager.py:136-142)."""
        evaluated = {_key(p) for p in self._get_checkpoints_with_results()}
        last_eval = self._clock()
        while True:
            if not os.path.isdir(self.model_dir):        # the training job may create it after the evaluation job started
                _log.info("Directory %s does not exist!", self.model_dir)
            else:
                todo = []
                for path in list_checkpoints(self.model_dir):
                    if _key(path) in evaluated:
                        continue
                    n = checkpoint_number(path)
                    if eval_every_steps and not (n > num_batched_steps and n % eval_every_steps < num_batched_steps):
                        continue
                    todo.append(path)
                for path in todo:
                    yield path
                if todo:
                    evaluated |= {_key(p) for p in todo}
                    last_eval = self._clock()
                    continue
            if self._clock() - last_eval > timeout or self.is_training_done():
                break
            self._sleep(POLL_SECONDS)


class TaskManagerWithCsvResults(TaskManager):
    """Task manager that keeps the results in ``scores.csv`` of the model directory (task_manager.py:160-202): the header is
    ``checkpoint_path, step`` and the sorted keys of the first result; Python floats are written as ``%.3f``."""

    def __init__(self, model_dir: str, score_file: Optional[str] = None, **kw) -> None:
        super().__init__(model_dir, **kw)
        self._score_file = os.path.join(self._model_dir, score_file or "scores.csv")

    @property
    def score_file(self) -> str:
        return self._score_file

    def _get_checkpoints_with_results(self):
        if not os.path.exists(self._score_file):
            return set()
        with open(self._score_file, newline="") as f:
            return {r["checkpoint_path"] for r in csv.DictReader(f)}

    def add_eval_result(self, checkpoint_path: str, result_dict: Dict[str, Any], default_value: int = -1) -> None:
        step = checkpoint_number(checkpoint_path)
        header = ["checkpoint_path", "step"] + sorted(result_dict)
        if not os.path.exists(self._score_file):
            os.makedirs(self._model_dir, exist_ok=True)
            with open(self._score_file, "w", newline="") as f:
                csv.DictWriter(f, fieldnames=header, extrasaction="ignore").writeheader()
        row = dict(checkpoint_path=checkpoint_path, step=str(step))
        for k, v in result_dict.items():
            row[k] = "{:.3f}".format(v) if isinstance(v, float) else v
        with open(self._score_file, "a", newline="") as f:
            csv.DictWriter(f, fieldnames=header, extrasaction="ignore").writerow(row)
