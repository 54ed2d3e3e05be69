"""st.regda.2rural: LoveDA Urban -> Rural (the names of the reference's configs/st/regda/2rural.py)."""
from configs.st.regda._surface import install

install(globals(), 'rural')
