"""spacedrive_amd -- MI355X-native content identification for Spacedrive.

Drop-in for sd-core's hot path:
  cas.generate_cas_id            core/src/object/cas.rs:23
  validation.file_checksum       core/src/object/validation/hash.rs:10
  file_identifier.*              core/src/object/file_identifier/mod.rs
  dedup.*                        identifier_job_step's Object grouping
  thumbnail_remover.*            core/src/object/thumbnail_remover.rs:236-367
  thumbnailer.*                  core/src/object/media/thumbnail/mod.rs:204-359
  indexer.*                      core/src/location/indexer/walk.rs:309-381,624-636
  dir_sizes.*                    what a directory holds, for file_path.size_in_bytes_bytes
  explorer.*                     core/src/api/search.rs:393-708 (paths, objects, counts)
  sync.*                         core/crates/sync/src/ingest.rs:114-233 (which ops apply)
All compute runs in libsdgpu.so (HIP kernels for gfx950); there is no CPU path.
"""
from ._native import Context, SdgpuError, default_context, load  # noqa: F401
from .cas import generate_cas_id  # noqa: F401
from .validation import file_checksum  # noqa: F401
from . import thumbnail_remover  # noqa: F401
from . import thumbnailer  # noqa: F401
from . import indexer  # noqa: F401
from . import dir_sizes  # noqa: F401
from . import explorer  # noqa: F401
from . import sync  # noqa: F401
from .thumbnail_remover import ThumbnailRemover, process_clean_up  # noqa: F401

__version__ = "0.1.0"
