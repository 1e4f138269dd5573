"""Device-side batchers with the reference's batch contract (`REC/data/dataset/{trainset,evalset,collate_fn}.py`)."""
from .batcher import Batch, SeqEvalBatcher, SeqStore, SeqTrainBatcher, batch_rows_cap  # noqa: F401
