"""Literal restatement of NumpyDataLoader.reset / generate_train_batch (toy_datamodule_3D.py:410-453; the LIDC module's
are the same lines) as far as they decide WHICH samples a batch holds -- nothing from values_amd.  One instance is one
worker of a MultiThreadedAugmenter: thread_id and number_of_threads_in_multithreaded are set by the caller."""
import numpy as np


class WorkerRef:
    def __init__(self, data, batch_size, training=True, thread_id=0, number_of_threads_in_multithreaded=1):
        self._data = list(data)
        self.num_restarted = 0
        self.current_position = 0
        self.was_initialized = False
        self.batch_size = batch_size
        self.training = training
        self.thread_id = thread_id
        self.number_of_threads_in_multithreaded = number_of_threads_in_multithreaded

    def reset(self):
        rs = np.random.RandomState(self.num_restarted)
        if self.training:
            rs.shuffle(self._data)
        self.was_initialized = True
        self.num_restarted = self.num_restarted + 1
        self.current_position = self.thread_id * self.batch_size

    def generate_train_batch(self):
        if not self.was_initialized:
            self.reset()
        idx = self.current_position
        if idx < len(self._data):
            self.current_position = idx + self.batch_size * self.number_of_threads_in_multithreaded
            samples = self._data[idx: min(len(self._data), idx + self.batch_size)]
        else:
            self.was_initialized = False
            return self.generate_train_batch()
        return samples


def drained(data, batch_size, training, num_workers, n_batches):
    """the batches of num_workers workers taken round-robin (the drain order values_amd.datamodule3d assumes)"""
    workers = [WorkerRef(data, batch_size, training, t, num_workers) for t in range(num_workers)]
    return [workers[k % num_workers].generate_train_batch() for k in range(n_batches)]
