"""Reading a training-data text file (``label<TAB>v1,v2,...`` per line) on the host: one line at a
time in Python, or in blocks of whole lines through a block parser - by default the device's,
``parse_training_text``, which is looked up here as this module's global when a file is read.
Nothing else in this module needs a GPU."""

import io
import os

import numpy as np

from ._text import parse_training_text


class TrainingDataError(ValueError):
    pass


_DATA_MESSAGES = {'label': 'a non-integer barcode class was encountered in {}',
                  'line': 'training signal not formatted correctly',
                  'sizes': 'inconsistent signal sizes in training data'}

TEXT_BLOCK_BYTES = 64 << 20
_TEXT_LOOKAHEAD = 8192      # a text-mode reader decodes this much at a time (io.TextIOWrapper)


def text_parse_route(parse=None):
    """'host' or 'gpu': ``parse``, or DEEPBINNER_TEXT_PARSE where it is None; unset: 'host'."""
    route = parse or os.environ.get('DEEPBINNER_TEXT_PARSE') or 'host'
    if route not in ('host', 'gpu'):
        raise ValueError("the training-data text route is 'host' or 'gpu', not {!r}".format(route))
    return route


def _training_line(line, number, path, input_size, messages):
    """One line of a training-data file, as the text-mode reader hands it out -> (label, int16 row,
    input_size: the row's where it was None); what does not fit raises TrainingDataError."""
    fields = line.strip().split('\t')
    if len(fields) != 2:
        raise TrainingDataError(messages['line'])
    label, values = fields
    if not label.lstrip('+-').isdigit():
        raise TrainingDataError(messages['label'].format(path))
    try:
        row = np.array(values.split(','), dtype=np.int64)
    except (ValueError, OverflowError):
        raise TrainingDataError(messages['line'])
    if row.size and (row.min() < -32768 or row.max() > 32767):
        raise TrainingDataError('line {} of {} holds signal values outside the int16 range'
                                .format(number, path))
    input_size = row.size if input_size is None else input_size
    if row.size != input_size:
        raise TrainingDataError(messages['sizes'])
    return int(label), row.astype(np.int16), input_size


def _read_training_data_host(path, input_size, messages):
    labels, rows = [], []
    with open(path, 'rt') as text:
        for number, line in enumerate(text, 1):
            label, row, input_size = _training_line(line, number, path, input_size, messages)
            labels.append(label)
            rows.append(row)
    if not rows:
        raise TrainingDataError(messages['line'])
    return np.stack(rows), np.array(labels, dtype=np.int32)


def training_text_blocks(path, block_bytes=None):
    """The file as blocks of whole lines, at most ``block_bytes`` each, cut behind a LF; a last
    line without a LF gets one.  A block is a view into one buffer that the next block reuses:
    it is good until the next one is asked for.  Yields None, and stops, at a line longer than a
    block."""
    block_bytes = block_bytes or TEXT_BLOCK_BYTES
    buffer = bytearray(block_bytes + 1)          # + 1: the LF a last line may lack
    view, held = memoryview(buffer), 0           # held: bytes of a line begun in the last read
    with open(path, 'rb') as raw:
        while True:
            got = raw.readinto(view[held:block_bytes])
            filled = held + got
            if not got:
                if held:
                    buffer[held] = 0x0a
                    yield view[:held + 1]
                return
            cut = buffer.rfind(b'\n', 0, filled) + 1
            if cut == 0:
                if filled >= block_bytes:
                    yield None
                    return
                held = filled
                continue
            yield view[:cut]
            held = filled - cut
            buffer[:held] = bytes(view[cut:filled])      # the line the cut left unfinished


def _refused_line(path, offset, length):
    """Line text as the text-mode reader would hand it out, for a line at ``offset`` that follows
    strict lines only; None where only a read of the whole file can tell (bytes outside ASCII in
    the line or in what that reader decodes along with it)."""
    with open(path, 'rb') as raw:
        raw.seek(offset)
        near = raw.read(length + _TEXT_LOOKAHEAD)
    if max(near, default=0) >= 0x80:
        return None
    return io.TextIOWrapper(io.BytesIO(near[:length]), encoding='ascii').readline()


def _read_training_data_blocks(path, input_size, messages, block_parser, block_bytes):
    asked = input_size
    with open(path, 'rt') as text:
        first = text.readline()
    if not first:
        raise TrainingDataError(messages['line'])
    _, _, input_size = _training_line(first, 1, path, input_size, messages)
    parts, lines_before, bytes_before = [], 0, 0
    for block in training_text_blocks(path, block_bytes):
        if block is None:
            return _read_training_data_host(path, asked, messages)
        samples, labels, kinds, first_bad = block_parser(block, input_size)
        if first_bad >= 0:
            block, start = bytes(block), 0
            for _ in range(first_bad):
                start = block.index(b'\n', start) + 1
            length = block.index(b'\n', start) + 1 - start
            line = _refused_line(path, bytes_before + start, length)
            if line is not None:
                # raises what the host route raises at this line, which is the first it refuses
                _training_line(line, lines_before + first_bad + 1, path, input_size, messages)
            # Python took what the grammar does not (or only it can tell): the host's route
            return _read_training_data_host(path, asked, messages)
        parts.append((samples, labels))
        lines_before += len(labels)
        bytes_before += len(block)
    if len(parts) == 1:
        return parts[0]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def strict_training_text(path, block_parser=None, block_bytes=None):
    """(int16 samples [n, L], int32 labels [n]) where EVERY line of the file is TEXT_OK with the
    first line's number of values, through ``block_parser`` (default parse_training_text); None
    otherwise, an empty file included - the caller then reads the file its own way."""
    block_parser = block_parser or parse_training_text
    with open(path, 'rb') as raw:
        input_size = raw.readline().count(b',') + 1
    if input_size > 1 << 20:
        return None
    parts = []
    for block in training_text_blocks(path, block_bytes):
        if block is None:
            return None
        samples, labels, _, first_bad = block_parser(block, input_size)
        if first_bad >= 0:
            return None
        parts.append((samples, labels))
    if len(parts) < 2:
        return parts[0] if parts else None
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def read_training_data(path, input_size=None, messages=None, parse=None, block_parser=None,
                       block_bytes=None):
    """A training-data text file (``label<TAB>v1,v2,...`` per line) as (int16 samples [n, L],
    int32 labels [n]), in one pass.  ``input_size`` None: the first line's.  A line that does not
    fit raises TrainingDataError; values outside int16 name the line, as in ``classify``.

    ``parse``: 'host' (one line at a time in Python), 'gpu' (the first line on the host, then
    blocks of ``block_bytes`` through ``block_parser``, by default parse_training_text; the first
    line a block refuses goes to the host's own code, which raises its error or, where it takes the
    line, reads the whole file), None: DEEPBINNER_TEXT_PARSE, unset 'host'.  Both routes return the
    same arrays and raise the same errors."""
    messages = messages or _DATA_MESSAGES
    if text_parse_route(parse) == 'host':
        return _read_training_data_host(path, input_size, messages)
    return _read_training_data_blocks(path, input_size, messages,
                                      block_parser or parse_training_text, block_bytes)
