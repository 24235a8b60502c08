//! The thumbnail remover's sweep (core/src/object/thumbnail_remover.rs:
//! 236-367, `process_clean_up`) with its database question -- `file_path.
//! cas_id IN (a shard directory's stems)`, a full table scan per directory and
//! library, the schema has no index on cas_id -- answered for the whole cache
//! by one call (`sdgpu_stale_thumbnails`): the thumbnails' cas keys against
//! the cas key columns the actor fetched from the loaded libraries.
//!
//! `remove_by_cas_ids` (:215-234) stays as it is: a host-only unlink loop.

use std::{
    collections::HashSet,
    ffi::OsStr,
    fs, io,
    path::{Path, PathBuf},
    ptr,
};

use sdgpu_sys as sys;

use crate::{check, Gpu};

/// One library's file_paths: the cas keys (little-endian first 8 bytes of the
/// cas_id, as `cas8`) and, when some rows have no cas_id, a byte per row.
pub struct Column<'a> {
    pub keys: &'a [u64],
    pub has_key: Option<&'a [u8]>,
}

/// Positions (in `thumb_keys`, listed directory by directory; `dir_start` =
/// ascending offsets from 0 to thumb_keys.len()) of the thumbnails no row of
/// `columns` owns, in list order, and their per-directory offsets.
pub fn stale_thumbnails(
    gpu: &Gpu,
    thumb_keys: &[u64],
    dir_start: &[u32],
    columns: &[Column<'_>],
) -> io::Result<(Vec<u32>, Vec<u32>)> {
    if dir_start.is_empty() || columns.iter().any(|c| c.has_key.map_or(false, |h| h.len() != c.keys.len())) {
        return Err(io::Error::from_raw_os_error(libc::EINVAL));
    }
    let keys: Vec<*const u64> = columns.iter().map(|c| c.keys.as_ptr()).collect();
    let has: Vec<*const u8> = columns.iter().map(|c| c.has_key.map_or(ptr::null(), |h| h.as_ptr())).collect();
    let rows: Vec<u64> = columns.iter().map(|c| c.keys.len() as u64).collect();
    let mut stale = vec![0u32; thumb_keys.len()];
    let mut stale_start = vec![0u32; dir_start.len()];
    let ctx = gpu.ctx();
    check(unsafe {
        sys::sdgpu_stale_thumbnails(*ctx, thumb_keys.as_ptr(), thumb_keys.len() as u64, dir_start.as_ptr(),
                                    (dir_start.len() - 1) as u32, keys.as_ptr(), has.as_ptr(), rows.as_ptr(),
                                    columns.len() as u32, stale.as_mut_ptr(), stale_start.as_mut_ptr())
    })?;
    stale.truncate(*stale_start.last().unwrap() as usize);
    Ok((stale, stale_start))
}

/// The cas key of a thumbnail stem, or None when the stem can equal no
/// database cas_id (anything but 16 characters of [0-9a-f]).
pub fn cas_key(stem: &str) -> Option<u64> {
    let b = stem.as_bytes();
    if b.len() != 16 || !b.iter().all(|c| matches!(c, b'0'..=b'9' | b'a'..=b'f')) {
        return None;
    }
    let mut raw = [0u8; 8];
    for (i, r) in raw.iter_mut().enumerate() {
        *r = u8::from_str_radix(&stem[2 * i..2 * i + 2], 16).ok()?;
    }
    Some(u64::from_le_bytes(raw))
}

#[derive(Default, Debug)]
pub struct Report {
    pub removed_files: Vec<PathBuf>,
    pub removed_dirs: Vec<PathBuf>,
}

struct Shard {
    path: PathBuf,
    thumbs: Vec<(String, PathBuf)>,
}

/// The walk of thumbnail_remover.rs:249-299; on an error the directories
/// scanned before it come back with it.
fn scan(thumbnails_directory: &Path) -> (Vec<Shard>, Option<io::Error>) {
    let mut shards = Vec::new();
    let res = (|| -> io::Result<()> {
        fs::create_dir_all(thumbnails_directory)?;
        for entry in fs::read_dir(thumbnails_directory)? {
            let entry = entry?;
            if !entry.metadata()?.is_dir() {
                continue;
            }
            let mut thumbs = Vec::new();
            for thumb in fs::read_dir(entry.path())? {
                let thumb_path = thumb?.path();
                if thumb_path.extension().and_then(OsStr::to_str).map_or(true, |ext| ext != "webp") {
                    continue;
                }
                let stem = thumb_path
                    .file_stem()
                    .and_then(OsStr::to_str)
                    .ok_or_else(|| io::Error::new(io::ErrorKind::InvalidData, "non UTF-8 thumbnail name"))?
                    .to_string();
                thumbs.push((stem, thumb_path));
            }
            shards.push(Shard { path: entry.path(), thumbs });
        }
        Ok(())
    })();
    (shards, res.err())
}

/// One sweep: scan, one `stale_thumbnails` call, unlink per directory in scan
/// order, remove a directory that held no thumbnail (:301-311) or whose every
/// thumbnail went (:353-362).  A stem that is no cas key is decided on the
/// host: stale unless the non-indexed set holds that string.  An error while
/// scanning directory k is returned after the directories before it were
/// swept, as the reference leaves them.
pub fn process_clean_up(
    gpu: &Gpu,
    thumbnails_directory: &Path,
    libraries: &[Column<'_>],
    non_indexed_cas_ids: &HashSet<String>,
) -> io::Result<Report> {
    let (shards, scan_err) = scan(thumbnails_directory);
    let mut remove: Vec<Vec<bool>> = shards
        .iter()
        .map(|s| s.thumbs.iter().map(|(stem, _)| !non_indexed_cas_ids.contains(stem)).collect())
        .collect();
    if !libraries.is_empty() {
        let mut keys = Vec::new();
        let mut place = Vec::new();
        let mut dir_start = vec![0u32];
        for (d, s) in shards.iter().enumerate() {
            for (j, (stem, _)) in s.thumbs.iter().enumerate() {
                if let Some(k) = cas_key(stem) {
                    keys.push(k);
                    place.push((d, j));
                }
            }
            dir_start.push(keys.len() as u32);
        }
        let extra: Vec<u64> = non_indexed_cas_ids.iter().filter_map(|c| cas_key(c)).collect();
        let mut columns: Vec<Column<'_>> =
            libraries.iter().map(|c| Column { keys: c.keys, has_key: c.has_key }).collect();
        columns.push(Column { keys: &extra, has_key: None });
        let (stale, _) = stale_thumbnails(gpu, &keys, &dir_start, &columns)?;
        for &(d, j) in &place {
            remove[d][j] = false;
        }
        for p in stale {
            let (d, j) = place[p as usize];
            remove[d][j] = true;
        }
    }
    let mut report = Report::default();
    for (s, gone) in shards.iter().zip(&remove) {
        for ((_, path), _) in s.thumbs.iter().zip(gone).filter(|(_, g)| **g) {
            fs::remove_file(path)?;
            report.removed_files.push(path.clone());
        }
        if gone.iter().all(|g| *g) {
            fs::remove_dir(&s.path)?;
            report.removed_dirs.push(s.path.clone());
        }
    }
    match scan_err {
        Some(e) => Err(e),
        None => Ok(report),
    }
}
