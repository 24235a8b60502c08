//! The thumbnailer's work list (core/src/object/media/thumbnail/mod.rs:
//! 204-359, `process`): its `fs::metadata` per row of
//! `<base>/<cas_id[0..2]>/<cas_id>.webp` (:254-256, :273) answered for a whole
//! column of file_paths by one call (`sdgpu_thumbnail_worklist`): the rows' cas
//! keys against the cas keys of the thumbnails on disk.  The explorer's
//! `has_local_thumbnail` (api/search.rs:540-547, library/library.rs:122-130) is
//! the same call in its presence-only mode.
//!
//! Deviation: two rows of one step that share a cas_id are one work row here
//! (the reference writes the same file twice and counts both as created).

use std::{io, ptr};

use sdgpu_sys as sys;

use crate::{check, Gpu};

/// One column of file_path rows in ascending id order: the cas keys
/// (little-endian first 8 bytes of the cas_id), a byte per row when some rows
/// have no cas_id, and the query's mask (location, extension list, sub-path).
pub struct Rows<'a> {
    pub keys: &'a [u64],
    pub has_key: Option<&'a [u8]>,
    pub eligible: Option<&'a [u8]>,
}

pub struct WorkList {
    /// The rows to generate, ordered by shard directory (the first cas byte),
    /// ascending inside a directory: the lowest candidate row of each cas_id.
    pub work: Vec<u32>,
    /// Offsets of the 256 shard directories into `work`; `[256]` = work.len().
    pub dir_start: Vec<u32>,
    /// Keyed rows whose thumbnail exists; keyed eligible rows; those of them
    /// whose thumbnail exists; work.len().
    pub stats: [u32; 4],
    /// `thumbnail_exists` per row.
    pub present: Vec<u8>,
}

fn masks_ok(rows: &Rows<'_>) -> bool {
    let n = rows.keys.len();
    rows.has_key.map_or(true, |h| h.len() == n) && rows.eligible.map_or(true, |e| e.len() == n)
}

/// `thumb_keys`: the cas keys of the thumbnails on disk (duplicates allowed).
pub fn work_list(gpu: &Gpu, thumb_keys: &[u64], rows: &Rows<'_>, regenerate: bool) -> io::Result<WorkList> {
    if !masks_ok(rows) {
        return Err(io::Error::from_raw_os_error(libc::EINVAL));
    }
    let n = rows.keys.len();
    let mut out = WorkList { work: vec![0u32; n], dir_start: vec![0u32; 257], stats: [0; 4], present: vec![0u8; n] };
    let flags = if regenerate { sys::SDGPU_THUMBS_REGENERATE } else { 0 };
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_thumbnail_worklist(*ctx, thumb_keys.as_ptr(), thumb_keys.len() as u64, rows.keys.as_ptr(),
                                      rows.has_key.map_or(ptr::null(), |h| h.as_ptr()),
                                      rows.eligible.map_or(ptr::null(), |e| e.as_ptr()), n as u64, flags,
                                      out.present.as_mut_ptr(), out.work.as_mut_ptr(),
                                      out.dir_start.as_mut_ptr(), out.stats.as_mut_ptr())
    })?;
    out.work.truncate(out.dir_start[256] as usize);
    Ok(out)
}

/// `Library::thumbnail_exists` for a page of rows: 1 where the row has a
/// cas_id and a thumbnail of it is on disk (presence-only mode, no grouping).
pub fn thumbnail_exists(gpu: &Gpu, thumb_keys: &[u64], keys: &[u64], has_key: Option<&[u8]>) -> io::Result<Vec<u8>> {
    if has_key.map_or(false, |h| h.len() != keys.len()) {
        return Err(io::Error::from_raw_os_error(libc::EINVAL));
    }
    let mut present = vec![0u8; keys.len()];
    let mut stats = [0u32; 4];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_thumbnail_worklist(*ctx, thumb_keys.as_ptr(), thumb_keys.len() as u64, keys.as_ptr(),
                                      has_key.map_or(ptr::null(), |h| h.as_ptr()), ptr::null(),
                                      keys.len() as u64, 0, present.as_mut_ptr(), ptr::null_mut(),
                                      ptr::null_mut(), stats.as_mut_ptr())
    })?;
    Ok(present)
}
