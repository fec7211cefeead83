"""The label font of the device renderer (`utils/draw.py`, `csrc/draw.hip`): a fixed-cell 1-bit bitmap font, no anti-aliasing.

The glyph shapes are the classic 5 x 7 dot-matrix set (character-LCD style), each dot drawn 2 x 2, in a cell that is
`ADVANCE` = 12 pixels wide and `HEIGHT` = 14 pixels tall: the glyph occupies columns 1..10 and rows 0..13, the baseline is the
cell's bottom row and there are no descenders (g, j, p, q, y are the squeezed dot-matrix forms).  `HEIGHT` is also the cap height
(`text_h`), next to the 13 px of Hershey Duplex at scale 0.6 that the reference measures, and `text_w = len(text) * ADVANCE`.
A label whose baseline-left is `(x1, y1 + 15)` covers rows `y1 + 2 .. y1 + 15` and columns `x1 .. x1 + text_w - 1`, inside its
plate `x1 .. x1 + text_w`, `y1 .. y1 + HEIGHT + 5`.

`FONT` is uint16 `[95][HEIGHT]` for the codes 0x20..0x7E; bit `x` of a row is column `x` of the cell.  Any other character is
drawn as `?` (`sanitize`).
"""
import numpy as np

ADVANCE = 12
HEIGHT = 14
FIRST, LAST = 0x20, 0x7E

# five column bytes per glyph, bit r = row r from the top (7 rows)
_DOTS_5X7 = (
    '0000000000' '00005F0000' '0007000700' '147F147F14' '242A7F2A12' '2313086462' '3649552250' '0005030000'   # sp ! " # $ % & '
    '001C224100' '0041221C00' '14083E0814' '08083E0808' '0050300000' '0808080808' '0060600000' '2010080402'   # ( ) * + , - . /
    '3E5149453E' '00427F4000' '4261514946' '2141454B31' '1814127F10' '2745454539' '3C4A494930' '0171090503'   # 0-7
    '3649494936' '064949291E' '0036360000' '0056360000' '0814224100' '1414141414' '0041221408' '0201510906'   # 8 9 : ; < = > ?
    '324979413E' '7E1111117E' '7F49494936' '3E41414122' '7F4141221C' '7F49494941' '7F09090901' '3E4149497A'   # @ A-G
    '7F0808087F' '00417F4100' '2040413F01' '7F08142241' '7F40404040' '7F020C027F' '7F0408107F' '3E4141413E'   # H-O
    '7F09090906' '3E4151215E' '7F09192946' '4649494931' '01017F0101' '3F4040403F' '1F2040201F' '3F4038403F'   # P-W
    '6314081463' '0708700807' '6151494543' '007F414100' '0204081020' '0041417F00' '0402010204' '4040404040'   # X Y Z [ \ ] ^ _
    '0001020400' '2054545478' '7F48444438' '3844444420' '384444487F' '3854545418' '087E090102' '0C5252523E'   # ` a-g
    '7F08040478' '00447D4000' '2040443D00' '7F10284400' '00417F4000' '7C04180478' '7C08040478' '3844444438'   # h-o
    '7C14141408' '081414187C' '7C08040408' '4854545420' '043F444020' '3C4040207C' '1C2040201C' '3C4030403C'   # p-w
    '4428102844' '0C5050503C' '4464544C44' '0008364100' '00007F0000' '0041360800' '0804081008'                # x y z { | } ~
)


def _build():
    cols = np.frombuffer(bytes.fromhex(''.join(_DOTS_5X7)), dtype=np.uint8).reshape(LAST - FIRST + 1, 5)
    font = np.zeros((LAST - FIRST + 1, HEIGHT), dtype=np.uint16)
    for g in range(cols.shape[0]):
        for c in range(5):
            for r in range(7):
                if (cols[g, c] >> r) & 1:
                    for dy in (0, 1):
                        font[g, 2 * r + dy] |= np.uint16(0b11 << (1 + 2 * c))
    font.setflags(write=False)
    return font


FONT = _build()


def sanitize(text):
    """The characters the font can draw: printable ASCII stays, anything else becomes `?`."""
    return ''.join(ch if FIRST <= ord(ch) <= LAST else '?' for ch in text)


def text_size(text):
    """(text_w, text_h) of a line, the role of cv2.getTextSize in the reference's draw_img."""
    return len(text) * ADVANCE, HEIGHT


def text_bitmap(text):
    """bool [HEIGHT][len(text) * ADVANCE]: the set pixels of a line of text."""
    text = sanitize(text)
    out = np.zeros((HEIGHT, len(text) * ADVANCE), dtype=bool)
    xs = np.arange(ADVANCE)
    for k, ch in enumerate(text):
        rows = FONT[ord(ch) - FIRST]
        out[:, k * ADVANCE:(k + 1) * ADVANCE] = (rows[:, None] >> xs[None, :]) & 1
    return out
