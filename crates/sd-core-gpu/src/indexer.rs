//! The indexer's rescan diff (core/src/location/indexer/walk.rs:309-381,
//! `filter_existing_paths`, and the per-directory `to_remove` query of
//! :624-636 / indexer/mod.rs:338-388): which walked entries are new, which
//! changed behind the library's back and which file_path rows are gone, for one
//! location by one call (`sdgpu_indexer_diff`).  Walking, the indexer rules and
//! the database writes stay with the caller.
//!
//! The keys are 64-bit stand-ins for (materialized_path, name, extension) and
//! for a directory's `materialized_path_for_children()`; the caller compares
//! the strings of every pair `(i, matched[i])` to make the answer exact.
//!
//! Deviation kept from the reference: a file replaced by a directory of the
//! same name is created again and its old row is not removed (state 3).

use std::{io, ptr};

use sdgpu_sys as sys;

use crate::{check, Gpu};

pub const IS_DIR: u8 = 1;
pub const ANCESTOR: u8 = sys::SDGPU_IDX_ANCESTOR as u8;
pub const NO_METADATA: u8 = sys::SDGPU_IDX_NO_METADATA as u8;
pub const MISS: u32 = sys::SDGPU_IDX_MISS;

pub const STATE_CREATE: u8 = 0;
pub const STATE_UNCHANGED: u8 = 1;
pub const STATE_UPDATE: u8 = 2;
pub const STATE_KIND_CHANGED: u8 = 3;

/// The walked entries (`indexed_paths`, ancestors included): `meta` holds
/// inode, device and modified_at (ns since the epoch) per entry.
pub struct Walked<'a> {
    pub keys: &'a [u64],
    pub flags: Option<&'a [u8]>,
    pub meta: &'a [[u64; 3]],
    /// Children-path keys of the directories whose listing was read.
    pub dir_keys: &'a [u64],
}

/// The location's file_path rows in ascending id order.
pub struct Rows<'a> {
    pub keys: &'a [u64],
    pub dir_keys: &'a [u64],
    pub flags: Option<&'a [u8]>,
    pub meta: &'a [[u64; 3]],
}

pub struct Diff {
    /// Walked entries to create (state 0 or 3), ascending.
    pub create: Vec<u32>,
    /// Walked entries whose row must be updated and its cas_id cleared.
    pub update: Vec<u32>,
    /// Rows to remove, ascending.
    pub remove: Vec<u32>,
    /// The lowest row with the entry's key, or `MISS`.
    pub matched: Vec<u32>,
    pub state: Vec<u8>,
    /// How many entries of `create` are KIND_CHANGED.
    pub kind_changed: u32,
}

pub fn diff(gpu: &Gpu, walked: &Walked<'_>, rows: &Rows<'_>) -> io::Result<Diff> {
    let (n_w, n_r) = (walked.keys.len(), rows.keys.len());
    if walked.meta.len() != n_w
        || walked.flags.map_or(false, |f| f.len() != n_w)
        || rows.dir_keys.len() != n_r
        || rows.meta.len() != n_r
        || rows.flags.map_or(false, |f| f.len() != n_r)
    {
        return Err(io::Error::from_raw_os_error(libc::EINVAL));
    }
    let mut out = Diff {
        create: vec![0u32; n_w],
        update: vec![0u32; n_w],
        remove: vec![0u32; n_r],
        matched: vec![0u32; n_w],
        state: vec![0u8; n_w],
        kind_changed: 0,
    };
    let mut counts = [0u32; 4];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_indexer_diff(*ctx, walked.keys.as_ptr(), walked.flags.map_or(ptr::null(), |f| f.as_ptr()),
                                walked.meta.as_ptr() as *const u64, n_w as u64, walked.dir_keys.as_ptr(),
                                walked.dir_keys.len() as u64, rows.keys.as_ptr(), rows.dir_keys.as_ptr(),
                                rows.flags.map_or(ptr::null(), |f| f.as_ptr()),
                                rows.meta.as_ptr() as *const u64, n_r as u64, out.matched.as_mut_ptr(),
                                out.state.as_mut_ptr(), out.create.as_mut_ptr(), out.update.as_mut_ptr(),
                                out.remove.as_mut_ptr(), counts.as_mut_ptr())
    })?;
    out.create.truncate(counts[0] as usize);
    out.update.truncate(counts[1] as usize);
    out.remove.truncate(counts[2] as usize);
    out.kind_changed = counts[3];
    Ok(out)
}
