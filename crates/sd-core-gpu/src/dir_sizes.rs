//! Recursive directory sizes of one location by one call (`sdgpu_dir_sizes`).
//! The reference stores the directory inode's size in
//! `file_path.size_in_bytes_bytes` for a directory row
//! (core/src/location/indexer/mod.rs:126-136, 215-225) and orders and shows by
//! that column (api/search.rs:85, api/locations.rs:66-100); this sums what the
//! directory holds instead.  The caller supplies the keys and the file sizes,
//! and writes `size_in_bytes_bytes` for directory rows if it wants them stored.
//!
//! The keys are 64-bit stand-ins for a row's own `materialized_path` and for a
//! directory's `materialized_path_for_children()`; the caller compares the
//! strings of every pair `(i, parent[i])` to make the answer exact, and re-keys
//! with another salt when `resolved < dirs`.

use std::{io, ptr};

use sdgpu_sys as sys;

use crate::{check, Gpu};

pub const IS_DIR: u8 = 1;
pub const MISS: u32 = sys::SDGPU_IDX_MISS;
pub const UNRESOLVED: u64 = sys::SDGPU_SIZE_UNRESOLVED;

/// The location's file_path rows in ascending id order.
pub struct Rows<'a> {
    /// Key of the row's own materialized_path.
    pub dir_keys: &'a [u64],
    /// Directory rows: key of materialized_path_for_children(); file rows: not read.
    pub self_keys: &'a [u64],
    /// Bit 0 is_dir; `None`: no directory rows.
    pub flags: Option<&'a [u8]>,
    /// size_in_bytes of file rows; not read for directory rows.
    pub sizes: &'a [u64],
}

pub struct DirSizes {
    /// The lowest directory row that owns the row's materialized_path, or `MISS`.
    pub parent: Vec<u32>,
    /// A file row's size; what a directory row holds, or `UNRESOLVED`.
    pub total: Vec<u64>,
    /// The file rows below a directory row (0xFFFFFFFF when unresolved).
    pub files: Vec<u32>,
    pub dirs: u64,
    /// `resolved < dirs`: a bad key or a collision, re-key with another salt.
    pub resolved: u64,
    pub top_level: u64,
    /// The sum of `total` over the rows without a parent.
    pub location_size: u64,
}

pub fn dir_sizes(gpu: &Gpu, rows: &Rows<'_>) -> io::Result<DirSizes> {
    let n = rows.dir_keys.len();
    if rows.sizes.len() != n
        || rows.flags.map_or(false, |f| f.len() != n || rows.self_keys.len() != n)
    {
        return Err(io::Error::from_raw_os_error(libc::EINVAL));
    }
    let mut out = DirSizes {
        parent: vec![0u32; n],
        total: vec![0u64; n],
        files: vec![0u32; n],
        dirs: 0,
        resolved: 0,
        top_level: 0,
        location_size: 0,
    };
    let mut counts = [0u64; 4];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_dir_sizes(*ctx, rows.dir_keys.as_ptr(),
                             if rows.flags.is_some() { rows.self_keys.as_ptr() } else { ptr::null() },
                             rows.flags.map_or(ptr::null(), |f| f.as_ptr()), rows.sizes.as_ptr(),
                             n as u64, out.parent.as_mut_ptr(), out.total.as_mut_ptr(),
                             out.files.as_mut_ptr(), counts.as_mut_ptr())
    })?;
    out.dirs = counts[0];
    out.resolved = counts[1];
    out.top_level = counts[2];
    out.location_size = counts[3];
    Ok(out)
}
